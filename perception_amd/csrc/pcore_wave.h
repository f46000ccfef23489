// pcore_wave.h -- wave-level primitives of the covariance and GICP kernels (one wave of 64 lanes; nothing here knows
// about either family): the wave's own LDS fence, wave-uniform values moved to SGPRs, an opaque zero that keeps
// per-lane addresses from being hoisted out of a loop, the integer min / max butterflies, and the double-precision
// sums of the oracle's shuffle-down tree formed in registers through v_permlane*_swap and DPP (wave_tree_sums for a
// set of values, wave_sum_lane0 for one).  The cross-lane instructions move 32 bits: a double goes through them as
// the two halves of d_halves / d_join.
#pragma once

#include <hip/hip_runtime.h>

namespace pcore {
namespace {

// LDS writes by some lanes of a wave visible to all its lanes (no block barrier: waves are independent)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a zero the compiler cannot see through: added to a per-lane index or an LDS pointer inside a loop, it keeps the
// address arithmetic (and loads through it) from being hoisted out of the loop into registers that get spilled
__device__ __forceinline__ int opaque_zero() {
    int z;
    asm volatile("s_mov_b32 %0, 0" : "=s"(z));
    return z;
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// the 32-bit halves of a double, and a double from its halves
__device__ __forceinline__ void d_halves(double v, unsigned& lo, unsigned& hi) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    lo = (unsigned)u;
    hi = (unsigned)(u >> 32);
}
__device__ __forceinline__ double d_join(unsigned lo, unsigned hi) {
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// a wave-uniform double moved to SGPRs (R, t of the pose being refined, the LM scalars)
// (the split spelled out, not through d_halves: with the split in a helper of any form -- references, a returned
// struct, one half per call -- the three GICP kernels compile to slightly different code around lm_iteration's solves)
__device__ __forceinline__ double uniform_d(double x) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return d_join(lo, hi);
}
__device__ __forceinline__ float uniform_f(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, x)));
}

// The wave shuffle-down tree of K <= 32 sums (GICP's 28 normal-equation sums; the oracle's order: node(l, off) =
// node(l, 2 off) + node(l + off, 2 off) for off = 32 ... 1, node(l, 64) = lane l's entry, so lane 0's sums
// ((x0 + x32) + (x16 + x48)) + ... ), computed in registers with the values split between the halves at every level:
// at offset o the lanes of each 2o-block pair two registers A, B; the lower half adds its partner's A and keeps value
// A, the upper half adds its partner's B and keeps value B.  Lane l then holds node(l mod o, o) of half as many
// values, so the wave does 16 + 8 + 4 + 2 + 1 + 1 adds instead of 28 x 6.  The sums are the tree's own (IEEE addition
// commutes), whichever lane forms them: value v ends on lane 2 v.  Offsets 32 and 16 swap halves with
// v_permlane32_swap / v_permlane16_swap, 8 and 4 use DPP row shifts written bank by bank, 2 and 1 quad permutations.
// (Round 3 transposed the partial sums through 7.4 KB of LDS per wave and summed them on 14 lanes: 5.6 k of ~36 k
// clocks per pose-iteration.)
template <int CTRL, int ROWS, int BANKS>
__device__ __forceinline__ double dpp_d(double old, double src) {
    unsigned olo, ohi, vlo, vhi;
    d_halves(old, olo, ohi);
    d_halves(src, vlo, vhi);
    const unsigned lo = __builtin_amdgcn_update_dpp(olo, vlo, CTRL, ROWS, BANKS, false);
    const unsigned hi = __builtin_amdgcn_update_dpp(ohi, vhi, CTRL, ROWS, BANKS, false);
    return d_join(lo, hi);
}
template <bool ROWS16>
__device__ __forceinline__ double swap_add(double a, double b) {  // offsets 32 (ROWS16 false) and 16
    unsigned alo, ahi, blo, bhi;
    d_halves(a, alo, ahi);
    d_halves(b, blo, bhi);
    if constexpr (ROWS16) {
        const auto l = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
        const auto h = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
        alo = l[0]; blo = l[1]; ahi = h[0]; bhi = h[1];
    } else {
        const auto l = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
        const auto h = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
        alo = l[0]; blo = l[1]; ahi = h[0]; bhi = h[1];
    }
    return d_join(alo, ahi) + d_join(blo, bhi);
}
template <int OFF>
__device__ __forceinline__ double bank_add(double a, double b) {  // offsets 8 (banks 0-1 | 2-3) and 4 (0, 2 | 1, 3)
    constexpr int LOW = OFF == 8 ? 0x3 : 0x5;
    const double t = dpp_d<0x110 + OFF, 0xf, 0xf ^ LOW>(dpp_d<0x100 + OFF, 0xf, LOW>(0.0, a), b);  // row_shl / row_shr
    const double u = dpp_d<0xE4, 0xf, 0xf ^ LOW>(a, b);                                            // own value
    return u + t;
}
// the K sums into out[0, K) (the wave's LDS), visible to every lane on return
template <int K>
__device__ __forceinline__ const double* wave_tree_sums(const double (&acc)[K], double* out, int lane) {
    static_assert(K > 16 && K <= 32, "28 sums: 16 register pairs at offset 32");
    double r[16];
#pragma unroll
    for (int k = 0; k < 16; k++) r[k] = swap_add<false>(acc[k], k + 16 < K ? acc[k + 16] : 0.0);
#pragma unroll
    for (int k = 0; k < 8; k++) r[k] = swap_add<true>(r[k], r[k + 8]);
#pragma unroll
    for (int k = 0; k < 4; k++) r[k] = bank_add<8>(r[k], r[k + 4]);
#pragma unroll
    for (int k = 0; k < 2; k++) r[k] = bank_add<4>(r[k], r[k + 2]);
    {  // offset 2: lanes 0-1 of a quad keep r0, lanes 2-3 r1
        const bool up = lane & 2;
        const double sel = up ? r[0] : r[1], own = up ? r[1] : r[0];
        r[0] = own + dpp_d<0x4E, 0xf, 0xf>(0.0, sel);  // quad_perm [2, 3, 0, 1]
    }
    r[0] = r[0] + dpp_d<0xB1, 0xf, 0xf>(0.0, r[0]);    // offset 1: quad_perm [1, 0, 3, 2]
    // (the slot's address formed here, not hoisted out of the iteration loop into a register that gets spilled)
    if (!(lane & 1) && (lane >> 1) < K) out[(lane >> 1) + opaque_zero()] = r[0];
    wave_lds_sync();
    return out;
}

// Lane 0's value of the wave shuffle-down tree x <- x + shfl_down(x, off), off = 32 ... 1 (the oracle's reduction
// order: ((x0 + x32) + (x16 + x48)) + ...), without the LDS pipe: the 32- and 16-lane levels through
// v_permlane32_swap / v_permlane16_swap (lane l < 32 receives lane l + 32, lane l of an even row lane l + 16), the
// 8 ... 1 levels through DPP row_shl (lane l of a row receives lane l + off).  Other lanes end with partial sums
// (read lane 0).
__device__ __forceinline__ double wave_sum_lane0(double x) {
    unsigned lo, hi;
    d_halves(x, lo, hi);
    x = x + d_join(__builtin_amdgcn_permlane32_swap(lo, lo, false, false)[1],
                   __builtin_amdgcn_permlane32_swap(hi, hi, false, false)[1]);
    d_halves(x, lo, hi);
    x = x + d_join(__builtin_amdgcn_permlane16_swap(lo, lo, false, false)[1],
                   __builtin_amdgcn_permlane16_swap(hi, hi, false, false)[1]);
    x = x + dpp_d<0x108, 0xf, 0xf>(0.0, x);  // row_shl:8
    x = x + dpp_d<0x104, 0xf, 0xf>(0.0, x);  // row_shl:4
    x = x + dpp_d<0x102, 0xf, 0xf>(0.0, x);  // row_shl:2
    x = x + dpp_d<0x101, 0xf, 0xf>(0.0, x);  // row_shl:1
    return x;
}

}  // namespace
}  // namespace pcore
