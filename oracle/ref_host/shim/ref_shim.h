// ref_shim.h -- what the reference's stage headers need to compile as plain host C++ and run serially.
// TEST INFRASTRUCTURE ONLY (oracle/ref_host/README.md).  Everything here is this project's own code: the CUDA
// qualifiers are empty, the launch indices are globals the driver sets before each call, the atomics are the serial
// operations, and Eigen / OpenCV / assimp are the few members model.h and compute_point_clouds.cuh name.
#pragma once
#include <algorithm>
#include <cassert>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <numeric>  // pcd_scene.cpp names std::iota and gets it through OpenCV's headers
#include <string>
#include <vector>

#define __host__
#define __device__
#define __global__

struct ref_dim3 {
    unsigned x = 1, y = 1, z = 1;
};
inline ref_dim3 blockIdx, blockDim, threadIdx, gridDim;

// One thread runs at a time, so each atomic is its plain read-modify-write; the old value is returned as CUDA does.
inline int atomicExch(int* p, int v) { int o = *p; *p = v; return o; }
inline int atomicMax(int* p, int v) { int o = *p; if (v > o) *p = v; return o; }
inline int atomicMin(int* p, int v) { int o = *p; if (v < o) *p = v; return o; }
inline int atomicOr(int* p, int v) { int o = *p; *p = o | v; return o; }
inline float atomicAdd(float* p, float v) { float o = *p; *p = o + v; return o; }
inline int atomicAdd(int* p, int v) { int o = *p; *p = o + v; return o; }

// cuda/utils.cuh reports the device memory in use; there is no device.
typedef int cudaError_t;
enum { cudaSuccess = 0 };
inline cudaError_t cudaMemGetInfo(size_t* free_byte, size_t* total_byte) { *free_byte = *total_byte = 0; return cudaSuccess; }
inline const char* cudaGetErrorString(cudaError_t) { return "no device"; }

// ---- Eigen: fixed-size float / double matrices, column-major as Eigen's default -----------------------------
// compute_point_clouds.cuh:27-32 multiplies a 3 x 3 block by a vector and adds a column.  Eigen's own evaluation
// order of that product depends on its version; the order here -- each row left to right -- is this project's
// (DESIGN.md section 6), so the bounded cloud's world point is pinned to the source, not to an Eigen release.
namespace Eigen {
template <typename T, int R, int C>
struct Matrix {
    T v[R * C];
    Matrix() : v{} {}
    Matrix(T a, T b, T c) : v{} { static_assert(R * C == 3, "three coefficients"); v[0] = a; v[1] = b; v[2] = c; }
    T& operator()(int r, int c) { return v[r + c * R]; }
    const T& operator()(int r, int c) const { return v[r + c * R]; }
    T& operator()(int i) { return v[i]; }
    const T& operator()(int i) const { return v[i]; }
    T& operator[](int i) { return v[i]; }
    const T& operator[](int i) const { return v[i]; }
    static Matrix Constant(T x) { Matrix m; for (T& e : m.v) e = x; return m; }
    template <int BR, int BC>
    Matrix<T, BR, BC> block(int r0, int c0) const {
        Matrix<T, BR, BC> b;
        for (int r = 0; r < BR; r++)
            for (int c = 0; c < BC; c++) b(r, c) = (*this)(r0 + r, c0 + c);
        return b;
    }
    Matrix& operator+=(const Matrix& o) { for (int i = 0; i < R * C; i++) v[i] = v[i] + o.v[i]; return *this; }
};
template <typename T>
inline Matrix<T, 3, 1> operator*(const Matrix<T, 3, 3>& m, const Matrix<T, 3, 1>& p) {
    Matrix<T, 3, 1> o;
    for (int r = 0; r < 3; r++) o[r] = (m(r, 0) * p[0] + m(r, 1) * p[1]) + m(r, 2) * p[2];
    return o;
}
typedef Matrix<float, 4, 4> Matrix4f;
typedef Matrix<double, 4, 4> Matrix4d;
typedef Matrix<float, 3, 1> Vector3f;
template <typename T, int R, int C>
inline std::ostream& operator<<(std::ostream& os, const Matrix<T, R, C>&) { return os; }
}  // namespace Eigen

// ---- OpenCV: a dense single-channel matrix, as much of cv::Mat as model.h and cuda_icp's scenes name ---------
// Rows are contiguous.  A copy copies the elements (OpenCV shares them; the sources here only read a copy).
// convertTo is this file's own code: CV_32S -> CV_16U by OpenCV's documented rule, saturate_cast<ushort>(int)
// (values below 0 become 0, values above 65535 become 65535).  It is pinned to that rule, not to an OpenCV build.
#define CV_16U 2
#define CV_32S 4
#define CV_32F 5
typedef unsigned short ushort;
namespace cv {
template <typename T> inline T saturate_cast(int v);
template <> inline ushort saturate_cast<ushort>(int v) { return (ushort)((unsigned)v <= 65535u ? v : v > 0 ? 65535 : 0); }
struct Mat {
    int rows = 0, cols = 0;
    Mat() {}
    Mat(int rows_, int cols_, int type) : rows(rows_), cols(cols_), type_(type), data_((size_t)rows_ * cols_ * elem(type)) {}
    int type() const { return type_; }
    template <typename T> T& at(int r, int c) { return *reinterpret_cast<T*>(data_.data() + offset<T>(r, c)); }
    template <typename T> const T& at(int r, int c) const { return *reinterpret_cast<const T*>(data_.data() + offset<T>(r, c)); }
    template <typename T> T* ptr() { return reinterpret_cast<T*>(data_.data()); }
    template <typename T> const T* ptr() const { return reinterpret_cast<const T*>(data_.data()); }
    void convertTo(Mat& dst, int rtype) const {
        if (type_ != CV_32S || rtype != CV_16U) { std::fprintf(stderr, "cv::Mat::convertTo: only CV_32S -> CV_16U\n"); std::abort(); }
        Mat out(rows, cols, CV_16U);
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++) out.at<ushort>(r, c) = saturate_cast<ushort>(at<int32_t>(r, c));
        dst = out;
    }

private:
    static size_t elem(int type) {
        if (type == CV_16U) return 2;
        if (type == CV_32S || type == CV_32F) return 4;
        std::fprintf(stderr, "cv::Mat: type %d is not in the shim\n", type);
        std::abort();
    }
    template <typename T> size_t offset(int r, int c) const {
        if (sizeof(T) != elem(type_) || r < 0 || r >= rows || c < 0 || c >= cols) {
            std::fprintf(stderr, "cv::Mat::at(%d, %d) outside %d x %d, or an element of the wrong size\n", r, c, rows, cols);
            std::abort();
        }
        return ((size_t)r * cols + c) * sizeof(T);
    }
    int type_ = CV_32F;
    std::vector<uint8_t> data_;
};
}  // namespace cv

// ---- assimp: model.h names these in members the stages never call --------------------------------------------
struct aiVector3D { float x = 0, y = 0, z = 0; };
struct aiMatrix4x4 { float m[16] = {}; };
struct aiScene;
struct aiNode;
