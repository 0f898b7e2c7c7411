// Stand-in for the RGB-D plane members of the reference's include/Frame.h (:170-200: ComputePlanesFromPEAC, mvBoundaryPoints, mvPlanePoints, plane_num_; the
// PCL point types of :57-58) that the stand-in Frame.h here leaves out (test infrastructure, see MapPoint.h here).  In the reference these are members of Frame
// itself; here they sit in a class derived from the stand-in Frame, so that the snippet of INTEGRATION.md row 2l compiles against the same declarations.
#ifndef FRAMEPLANES_H
#define FRAMEPLANES_H

#include <vector>

#include "Frame.h"

namespace pcl {
struct PointXYZRGB { float x = 0, y = 0, z = 0; unsigned rgba = 0; };
template <class PointT>
struct PointCloud { std::vector<PointT> points; };
}  // namespace pcl

namespace ORB_SLAM2 {
class FrameWithPlanes : public Frame {
public:
    typedef pcl::PointXYZRGB PointT;
    typedef pcl::PointCloud<PointT> PointCloud;
    void ComputePlanesFromPEAC(const cv::Mat& imDepth);
    std::vector<PointCloud> mvBoundaryPoints, mvPlanePoints;
    int plane_num_ = 0;
};
}  // namespace ORB_SLAM2
#endif  // FRAMEPLANES_H
