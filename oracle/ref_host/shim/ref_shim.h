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

// ---- OpenCV / assimp: model.h names them in members the stages never call -----------------------------------
#define CV_32F 5
namespace cv {
struct Mat {
    int type() const { return CV_32F; }
    template <typename T> T at(int, int) const { return T(); }
};
}  // namespace cv
struct aiVector3D { float x = 0, y = 0, z = 0; };
struct aiMatrix4x4 { float m[16] = {}; };
struct aiScene;
struct aiNode;
