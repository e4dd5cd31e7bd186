// cv_compat.h -- the handful of OpenCV value types that cross the adjustBundle() boundary.
//
// The reference's data model (SfMToyLib/SfMCommon.h:55-99) is built on cv::Matx34f, cv::Point3f,
// cv::Point2f and a CV_32F 3x3 cv::Mat.  OpenCV is not installable in this environment, so this header
// provides layout- and API-compatible stand-ins for exactly the members adjustBundle() touches
// (BA.cpp:111-221), plus CV_8U descriptor matrices for matchFeatures() and CV_8U / CV_8UC3 images for extractFeatures().  Building with -DSFMBA_HAVE_OPENCV uses the real headers instead; the shim source
// is identical in both cases.
#pragma once
#ifdef SFMBA_HAVE_OPENCV
#include <opencv2/core/core.hpp>
#include <opencv2/features2d/features2d.hpp>
#else
#include <cstring>
#include <vector>

enum { CV_8U = 0, CV_32F = 5, CV_8UC3 = 16, CV_32FC3 = 21 };     // OpenCV's type codes (CV_8UC3: three interleaved bytes, BGR; CV_32FC3: three floats); global, as OpenCV's macros are

namespace cv {

template <typename T, int M, int N>
struct Matx {
    T val[M * N];
    Matx() { for (int i = 0; i < M * N; ++i) val[i] = T(0); }
    static Matx eye() { Matx m; for (int i = 0; i < (M < N ? M : N); ++i) m(i, i) = T(1); return m; }
    T& operator()(int r, int c) { return val[r * N + c]; }
    const T& operator()(int r, int c) const { return val[r * N + c]; }
    template <int M1, int N1>
    Matx<T, M1, N1> get_minor(int r0, int c0) const {
        Matx<T, M1, N1> m;
        for (int r = 0; r < M1; ++r) for (int c = 0; c < N1; ++c) m(r, c) = (*this)(r0 + r, c0 + c);
        return m;
    }
    Matx<T, N, M> t() const {
        Matx<T, N, M> m;
        for (int r = 0; r < M; ++r) for (int c = 0; c < N; ++c) m(c, r) = (*this)(r, c);
        return m;
    }
};
typedef Matx<float, 3, 4> Matx34f;
typedef Matx<float, 3, 3> Matx33f;

template <typename T> struct Point_ { T x, y; Point_() : x(0), y(0) {} Point_(T x_, T y_) : x(x_), y(y_) {} };
template <typename T> struct Point3_ { T x, y, z; Point3_() : x(0), y(0), z(0) {} Point3_(T x_, T y_, T z_) : x(x_), y(y_), z(z_) {} };
typedef Point_<float> Point2f;
typedef Point3_<float> Point3f;

struct KeyPoint { Point2f pt; float size = 0, angle = -1, response = 0; int octave = 0, class_id = -1; };
struct DMatch { int queryIdx = -1, trainIdx = -1, imgIdx = -1; float distance = 0; DMatch() {} DMatch(int q, int t, float d) : queryIdx(q), trainIdx(t), distance(d) {} };

// Dense row-major matrix, continuous, zero-initialised: a CV_32F one is what Intrinsics::K needs (K.at<float>(r, c),
// BA.cpp:138,151-153,188-189), a CV_8U one holds binary descriptors (Features::descriptors, one row per key point) or a gray
// image, a CV_8UC3 one a BGR image (cols counts pixels, a row is 3 cols bytes), a CV_32FC3 one a normal map (a row is 3 cols floats).
class Mat {
public:
    Mat() : rows(0), cols(0), type_(CV_32F) {}
    Mat(int r, int c) : Mat(r, c, CV_32F) {}
    Mat(int r, int c, int type) : rows(r), cols(c), type_(type), data_(((size_t)r * c * elem(type) + 3) / 4, 0.0f) {}
    template <typename T> T& at(int r, int c) { return ptr<T>(r)[c]; }
    template <typename T> const T& at(int r, int c) const { return ptr<T>(r)[c]; }
    template <typename T> T* ptr(int r) { return reinterpret_cast<T*>(bytes() + (size_t)r * cols * elem(type_)); }
    template <typename T> const T* ptr(int r) const { return reinterpret_cast<const T*>(bytes() + (size_t)r * cols * elem(type_)); }
    int type() const { return type_; }
    bool empty() const { return data_.empty(); }
    int rows, cols;
private:
    static size_t elem(int type) { return type == CV_8U ? 1 : type == CV_8UC3 ? 3 : type == CV_32FC3 ? 12 : 4; }
    unsigned char* bytes() { return reinterpret_cast<unsigned char*>(data_.data()); }
    const unsigned char* bytes() const { return reinterpret_cast<const unsigned char*>(data_.data()); }
    int type_;
    std::vector<float> data_;      // float words whatever the type: 4-byte aligned storage
};

}  // namespace cv
#endif
