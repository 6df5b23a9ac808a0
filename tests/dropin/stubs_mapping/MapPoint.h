// Test stub of the reference's MapPoint for the mapping-side search: SearchForTriangulation only asks
// whether a keypoint has one.  Written for the test.
#pragma once
namespace ygz {
class MapPoint {};
}  // namespace ygz
