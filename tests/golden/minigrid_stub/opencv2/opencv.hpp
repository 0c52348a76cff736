// Compile-only stand-in for the one OpenCV call of the reference's MiniGrid renderer
// (cv::resize in Render).  Rendering is not part of the fixtures: calling it aborts.
#pragma once
#include <cstdlib>
namespace cv {
constexpr int CV_8UC3 = 16, INTER_AREA = 3;
struct Size { Size(int, int) {} };
struct Mat { Mat(int, int, int, void*) {} };
inline void resize(const Mat&, Mat&, Size, double, double, int) { std::abort(); }
}  // namespace cv
using cv::CV_8UC3;
