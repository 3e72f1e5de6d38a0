// The two OpenCV names dbscan.cpp uses, as OpenCV defines their behaviour: cv::Point_ difference in the element type and
// cv::norm of a point = sqrt((double)x*x + (double)y*y); cv::KeyPoint with OpenCV's fields.  Lets the reference's own
// dbscan.cpp compile without OpenCV for tests/golden/make_ref_dbscan_golden.py.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace cv {
template <typename T> struct Point_ {
    T x, y;
    Point_() : x(0), y(0) {}
    Point_(T a, T b) : x(a), y(b) {}
};
template <typename T> inline Point_<T> operator-(const Point_<T> &a, const Point_<T> &b) { return Point_<T>(a.x - b.x, a.y - b.y); }
typedef Point_<float> Point2f;
template <typename T> inline double norm(const Point_<T> &p) { return std::sqrt((double)p.x * p.x + (double)p.y * p.y); }
struct KeyPoint {
    Point2f pt;
    float size = 0, angle = -1, response = 0;
    int octave = 0, class_id = -1;
};
} // namespace cv
