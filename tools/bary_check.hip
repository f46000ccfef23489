// bary_check.hip -- checker (test infrastructure, not product code): the fragment test's barycentrics without the
// reference's three halves (pcore::frag_barycentrics<true>, pcore_fdiv.h) against the reference form
// (frag_barycentrics<false>), bit for bit, on the GPU, over inputs inside the bound pcore_fdiv.h documents for a fastdiv
// pose: every coordinate a multiple of 2^-25 of magnitude below 2^56, sample centres non-negative integers.
//
// Inputs: 2^26 (triangle, sample) pairs per launch from a counter-based hash -- coordinates n * 2^e with 24-bit n and
// e over [-25, 32] (the whole bound), typical screen coordinates with fine fractions, vertices that coincide or share a
// coordinate (zero areas), collinear vertices, triangles a few 2^-25 across (far below 10^-3 pixel), and samples on a
// vertex or exactly on an edge.  The inside test is compared as well.
// Prints one JSON line {"pairs": N, "mismatches": M, "zero_area": Z, "nan": K, "inside": I}; exit status 1 on any
// mismatch.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o tools/bin/bary_check tools/bary_check.hip
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../perception_amd/csrc/pcore_fdiv.h"

#pragma clang fp contract(off)

__device__ __forceinline__ uint32_t mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// a coordinate inside the bound: a multiple of 2^-25 below 2^56 in magnitude
__device__ __forceinline__ float coord(uint32_t h, uint32_t kind) {
    const float n = (float)(h & 0xffffffu);  // 24 bits: exact
    const float s = (h >> 31) ? -1.0f : 1.0f;
    if (kind < 8) return s * n * 0x1p-14f;                               // typical: |v| < 1024, steps of 2^-14
    if (kind < 10) return s * ldexpf(n, -25 + (int)((h >> 24) & 63u) % 58);  // the whole bound: e in [-25, 32]
    if (kind < 12) return s * (float)((h >> 4) & 0x3ffu);                // integers (sample centres' grid)
    if (kind < 14) return s * n * 0x1p-25f;                              // the finest grid, |v| < 0.5
    return (float)((h >> 4) & 0x3ffu) + (float)(h & 15u) * 0x1p-25f;     // an integer plus a few 2^-25
}

__device__ __forceinline__ bool same(float a, float b) {
    return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
}

__global__ void check(uint32_t seed, unsigned long long* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t h[9];
    for (int k = 0; k < 9; k++) h[k] = mix(i * 9u + (uint32_t)k + seed * (2u * (uint32_t)k + 3u));
    const uint32_t kind = h[8] & 15u;
    float A0 = coord(h[0], kind), A1 = coord(h[1], kind), B0 = coord(h[2], kind), B1 = coord(h[3], kind);
    float C0 = coord(h[4], kind), C1 = coord(h[5], kind);
    float P0 = (float)((h[6] >> 8) & 0x3fffu), P1 = (float)((h[7] >> 8) & 0x3fffu);  // sample centres: integers
    const uint32_t shape = (h[8] >> 4) & 31u;
    if (shape == 0) { B0 = A0; B1 = A1; }                                  // two vertices coincide: zero area
    else if (shape == 1) { C0 = A0; C1 = A1; B0 = A0; B1 = A1; }           // a point
    else if (shape == 2) { B1 = A1; C1 = A1; }                             // collinear, axis-parallel
    else if (shape == 3 && (kind < 8 || kind >= 10)) {  // collinear up to rounding (not at the bound's edge: C = 2B - A)
        C0 = A0 + (B0 - A0) + (B0 - A0);
        C1 = A1 + (B1 - A1) + (B1 - A1);
    }
    else if (shape < 8) {  // a sliver a few 2^-25 across next to A (A below 2^24 * 2^-25 keeps the grid)
        A0 = (float)(h[0] & 0xffffu) * 0x1p-25f; A1 = (float)(h[1] & 0xffffu) * 0x1p-25f;
        B0 = A0 + (float)(h[2] & 7u) * 0x1p-25f; B1 = A1 + (float)(h[3] & 7u) * 0x1p-25f;
        C0 = A0 + (float)(h[4] & 7u) * 0x1p-25f; C1 = A1 + (float)(h[5] & 7u) * 0x1p-25f;
    } else if (shape < 12) {  // integer vertices: samples fall exactly on vertices and edges
        A0 = (float)(h[0] & 31u); A1 = (float)(h[1] & 31u); B0 = (float)(h[2] & 31u); B1 = (float)(h[3] & 31u);
        C0 = (float)(h[4] & 31u); C1 = (float)(h[5] & 31u);
        P0 = (float)(h[6] & 31u); P1 = (float)(h[7] & 31u);
        if (shape == 8) { P0 = A0; P1 = A1; }
        if (shape == 9) { P0 = (A0 + B0) * 0.5f; P1 = (A1 + B1) * 0.5f; P0 = floorf(P0); P1 = floorf(P1); }
    } else if (shape < 16) {  // samples near a typical triangle
        P0 = floorf(fabsf(A0)) + (float)(h[6] & 7u);
        P1 = floorf(fabsf(A1)) + (float)(h[7] & 7u);
    }
    float b0, g0, b1, g1;
    pcore::frag_barycentrics<false>(A0, A1, B0, B1, C0, C1, P0, P1, b0, g0);
    pcore::frag_barycentrics<true>(A0, A1, B0, B1, C0, C1, P0, P1, b1, g1);
    const float a0 = 1.0f - b0 - g0, a1 = 1.0f - b1 - g1;
    const bool in0 = !(a0 < -0.0f || b0 < -0.0f || g0 < -0.0f || a0 > 1.0f || b0 > 1.0f || g0 > 1.0f);
    const bool in1 = !(a1 < -0.0f || b1 < -0.0f || g1 < -0.0f || a1 > 1.0f || b1 > 1.0f || g1 > 1.0f);
    if (!same(b0, b1) || !same(g0, g1) || in0 != in1) atomicAdd(&out[0], 1ull);
    const float Y = (C0 - A0) * (B1 - A1) - (B0 - A0) * (C1 - A1);
    if (Y == 0.0f) atomicAdd(&out[1], 1ull);
    if (b0 != b0 || g0 != g0) atomicAdd(&out[2], 1ull);
    if (in0) atomicAdd(&out[3], 1ull);
}

int main() {
    unsigned long long *d, h[4] = {0, 0, 0, 0};
    if (hipMalloc(&d, 32) != hipSuccess) return 2;
    if (hipMemset(d, 0, 32) != hipSuccess) return 2;
    const int launches = 8, blocks = 1 << 18, threads = 256;
    for (int l = 0; l < launches; l++)
        hipLaunchKernelGGL(check, dim3(blocks), dim3(threads), 0, 0, (uint32_t)l * 0x9e3779b9u + 1u, d);
    if (hipDeviceSynchronize() != hipSuccess) return 2;
    if (hipMemcpy(h, d, 32, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    printf("{\"pairs\": %.0f, \"mismatches\": %llu, \"zero_area\": %llu, \"nan\": %llu, \"inside\": %llu}\n",
           (double)launches * blocks * threads, h[0], h[1], h[2], h[3]);
    return h[0] == 0 ? 0 : 1;
}
