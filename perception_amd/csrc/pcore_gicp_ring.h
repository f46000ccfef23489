// pcore_gicp_ring.h -- rings of float transforms in a wave's LDS, compared as bit patterns by the whole wave at once:
// a pose's transform rounded to float (xform_float: what the correspondence queries are computed from) is spread
// over four lanes per slot (xf_lane_words), and one ballot tells which of 16 slots hold it (ring_match16).  CycleExit
// is the cycle exit of pcore_gicp_math.h (cycle_update / cycle_member) on a 32-slot ring; gicp_kernel's correspondence
// history keeps its 16-slot ring in the same layout (in the kernel's body: it sits at the register budget).
#pragma once

#include "pcore_gicp_math.h"
#include "pcore_wave.h"

namespace pcore {
namespace {

// float(R), float(t) of a wave-uniform double transform, in SGPRs
__device__ __forceinline__ void xform_float(const double (&R)[3][3], const double (&t)[3], float (&Rf)[3][3],
                                            float (&tf)[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) Rf[r][c] = uniform_f((float)R[r][c]);
        tf[r] = uniform_f((float)t[r]);
    }
}

// A 16-slot ring of float transforms in LDS (the correspondence history and the cycle exit): lane l holds components
// 3 (l & 3) + v (v = 0, 1, 2) of slot l >> 2 in word v (R rows 0..2, then t), as bit patterns (-0 != +0, NaN == NaN).
__device__ __forceinline__ void xf_lane_words(const float (&Rf)[3][3], const float (&tf)[3], int sub, unsigned& b0,
                                              unsigned& b1, unsigned& b2) {
    const float c0 = sub == 0 ? Rf[0][0] : sub == 1 ? Rf[1][0] : sub == 2 ? Rf[2][0] : tf[0];
    const float c1 = sub == 0 ? Rf[0][1] : sub == 1 ? Rf[1][1] : sub == 2 ? Rf[2][1] : tf[1];
    const float c2 = sub == 0 ? Rf[0][2] : sub == 1 ? Rf[1][2] : sub == 2 ? Rf[2][2] : tf[2];
    b0 = __builtin_bit_cast(unsigned, c0);
    b1 = __builtin_bit_cast(unsigned, c1);
    b2 = __builtin_bit_cast(unsigned, c2);
}

// bit s set: all four lanes of slot s hold (b0, b1, b2) (the lanes' current words hv0..hv2)
__device__ __forceinline__ unsigned ring_match16(unsigned b0, unsigned b1, unsigned b2, unsigned hv0, unsigned hv1,
                                                 unsigned hv2) {
    unsigned long long eq = __ballot(b0 == hv0 && b1 == hv1 && b2 == hv2);
    eq = eq & (eq >> 1) & (eq >> 2) & (eq >> 3) & 0x1111111111111111ull;  // bit 4s: slot s
    eq = (eq | (eq >> 3)) & 0x0303030303030303ull;                         // gather bit 4s to bit s
    eq = (eq | (eq >> 6)) & 0x000f000f000f000full;
    eq = (eq | (eq >> 12)) & 0x000000ff000000ffull;
    eq = (eq | (eq >> 24)) & 0xffffull;
    return (unsigned)eq;
}

// The cycle exit (pcore_gicp_math.h cycle_update) of one wave: the last 32 float transforms T_f(j) in slot
// (j - 1) % 32 of an LDS ring of two 16-slot banks (words 0..2: slots 0..15, words 3..5: slots 16..31, each bank laid out
// as xf_lane_words), the slots written so far and the run counters.
static_assert(gicpm::kCycleLags == 32, "CycleExit holds 32 slots");
constexpr int kCycleRingWords = 6 * 64;

struct CycleExit {
    unsigned* ring;  // kCycleRingWords, this wave's
    unsigned written;
    gicpm::CycleRun run;

    __device__ __forceinline__ void start(int lane) {  // T_f(1) = float(identity) in slot 0
        // lane l < 4 writes row l of I (t = 0 for l = 3): word v is 1.0f where v == l; formed here from an opaque lane
        // index, or the compiler hoists the words and addresses out of the persistent pose loop and holds 4 VGPRs
        const int l = lane + opaque_zero();
        if (l < 4) {  // every lane reads back only the words it wrote itself
            ring[l] = l == 0 ? 0x3f800000u : 0u;
            ring[64 + l] = l == 1 ? 0x3f800000u : 0u;
            ring[128 + l] = l == 2 ? 0x3f800000u : 0u;
        }
        written = 1u;
        run = {0, 0, 0};
    }

    // after iteration `iters`' accepted step (iters < max_iter): T_f(iters + 1) = float(R, t).  Returns -1, or the ring
    // slot of the cycle member the pose stops with (read by `member` once the loop has ended).
    __device__ __forceinline__ int step(const double (&R)[3][3], const double (&t_)[3], int iters, int max_iter,
                                        int window, bool inert, int lane_) {
        const int lane = lane_ + opaque_zero();  // per-lane values formed here, not hoisted out of the iteration loop
        float Rf[3][3], tf[3];
        xform_float(R, t_, Rf, tf);
        unsigned b0, b1, b2;
        xf_lane_words(Rf, tf, lane & 3, b0, b1, b2);
        const int cur = iters + 1, c0 = (cur - 1) & 31, bank = c0 >> 4;
        const unsigned m0 = ring_match16(b0, b1, b2, ring[lane], ring[64 + lane], ring[128 + lane]);
        const unsigned m1 = ring_match16(b0, b1, b2, ring[192 + lane], ring[256 + lane], ring[320 + lane]);
        const unsigned m = (m0 | (m1 << 16)) & written;
        // lag q lives in slot (c0 - q) % 32: in the doubled mask at c0 + 32 - q, so the smallest lag is the highest bit
        const unsigned long long mm = (unsigned long long)m | ((unsigned long long)m << 32);
        const unsigned t = (unsigned)(mm >> c0);
        const int p = t ? 32 - (31 - __builtin_clz(t)) : 0;
        if ((lane >> 2) == (c0 & 15)) {
            unsigned* w = ring + 192 * bank + lane;
            w[0] = b0;
            w[64] = b1;
            w[128] = b2;
        }
        written |= 1u << c0;
        if (!gicpm::cycle_update(run, p, inert, window)) return -1;
        return (gicpm::cycle_member(cur, p, max_iter) - 1) & 31;
    }

    // the float transform of ring slot s as the pose's result (after the loop: it is written back, not iterated on; the
    // ring was written by the whole wave, read here by every lane)
    __device__ __forceinline__ void member(int s, double (&R)[3][3], double (&t)[3]) {
        wave_lds_sync();
        const unsigned* w = ring + 192 * (s >> 4) + 4 * (s & 15);
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int v = 0; v < 3; v++) {
                const double f = (double)__builtin_bit_cast(float, w[64 * v + r]);
                if (r < 3) R[r][v] = f;
                else t[v] = f;
            }
    }
};

}  // namespace
}  // namespace pcore
