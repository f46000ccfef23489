// pcore_fused.hip -- stage COST of the render-and-compare hot path on CDNA4 (gfx950): fused sampled render +
// unproject + 1-NN + cost.  Float semantics and the helpers shared with the other stages: pcore_raster.h.
//
// Kernels
//   fused_cost_kernel      one workgroup per candidate pose; z-buffer of the stride-sampled pixels kept in LDS,
//                          vertex-ring stream transform, per-wave compaction of the (triangle, sample) work, source
//                          occlusion, unprojection, fixed-radius 1-NN and the three per-pose costs.  No per-pose HBM
//                          traffic except 64 B of pose in and 12 B of costs out.
//   window_probe_kernel    the tier histogram of a batch's pose windows (pose_window), for the first tile choice.
//   render_cloud_kernel    stage CLOUD into per-pose scratch slots (the ICPs' source clouds): the same raster, then
//                          the reference's row-major compaction.
// The full-resolution parity renderer is pcore_render.hip; the cloud / depth2cloud_global kernels, the source
// sampler and select_kernel are pcore_cloud.hip.
#include "pcore_raster.h"
#include "pcore_colour.h"
#include "pcore_fused_probe.h"

#include <algorithm>
#include <type_traits>

#pragma clang fp contract(off)

namespace pcore {

constexpr int kWaves = kFusedWaves;  // waves per fused / cloud workgroup (one pose)
constexpr int kThreads = kWaves * kWave;
// per-wave circular ring of queued triangle records, flushed 64 at a time: after every full flush fewer than
// 64 remain and a batch appends at most 64, so 128 never overflows; phase 2 reuses it as a point queue of
// up to 127 (tile index, kx | ky << 16) pairs
constexpr int kRecCap = 128;
// per-wave record ring stride.  The two spare records are unused (one was the target of a branch-free queue store that
// measured no faster), but the stride places every wave's ring, and the buffers carved after
// it, on the LDS banks: it is part of the measured layout and stays.
constexpr int kRecStride = kRecCap + 2;
constexpr int kSmallK = 4;    // triangles touching <= kSmallK samples are queued; larger ones are
                              // processed cooperatively by the whole wave

struct TriRec {  // a triangle in registers: screen-space vertices, camera z (or its reciprocal: raster_sample, RZ)
    float a0, a1, b0, b1, c0, c1, z0, z1, z2;
};
// A queued (triangle, sample) pair in the LDS record ring (8 bytes): x = the triangle's slot word (its three
// vertex-ring slots i0 | i1 << 9 | i2 << 18), y = the sample kx | ky << 16.

template <int STRIDE>
__device__ __forceinline__ int sdiv(int v, int s) {
    if constexpr (STRIDE > 0) return v / STRIDE;
    else return v / s;
}

// Sample window of a triangle with exact reference bbox (bmin, bmax): kx in [kx0, kx0+nx),
// ky in [ky0, ky0+ny) where the sampled output pixel is (kx*s, ky*s) and raster row P1 = H-1-ky*s.
template <int STRIDE>
__device__ __forceinline__ int sample_window(const float (&bmin)[2], const float (&bmax)[2], int s, int H, int& kx0,
                                             int& ky0, int& nx, int& ny) {
    int lo0, hi0, lo1, hi1;
    if (!loop_bounds(bmin[0], bmax[0], lo0, hi0)) return 0;
    if (!loop_bounds(bmin[1], bmax[1], lo1, hi1)) return 0;
    const int ss = STRIDE > 0 ? STRIDE : s;
    kx0 = sdiv<STRIDE>(lo0 + ss - 1, s);
    const int kx1 = sdiv<STRIDE>(hi0, s);
    // output rows y = H-1-P1 for P1 in [lo1, hi1]
    ky0 = sdiv<STRIDE>(H - 1 - hi1 + ss - 1, s);
    const int ky1 = sdiv<STRIDE>(H - 1 - lo1, s);
    nx = kx1 - kx0 + 1;
    ny = ky1 - ky0 + 1;
    if (nx <= 0 || ny <= 0) return 0;
    return nx * ny;
}

struct FusedSmem {
    int32_t* zbuf;  // tile samples
    float2* vxy;    // kWaves * kVRing * 64: screen (x, y) of the wave's vertex ring
    float* vz;      // kWaves * kVRing * 64: camera z (cm); v_rcp_f32 of it in the depth pass of a fastdiv pose
    uint2* vbd;     // kWaves * 2 * 64: packed int16 sample-window bounds of the last two passes
    uint2* ring;    // kWaves * kRecStride queued triangle records (phase 1); int32 point queues in phase 2
    uint32_t* ring_id;  // kWaves * kRecStride original triangle ids (colour id pass only)
    uint32_t* bitmap;
    int32_t* counters;  // [0] bad, [1] explained, [2] points; [4..10] the pose window (x0, y0, nx, ny, fastdiv, sparse,
                        // interior)
};
constexpr int kRingSlots = kVRing * kWave;
static_assert(kRingSlots <= (1 << kRingSlotBits), "vertex ring slots must fit the 9-bit triangle indices");
static_assert(kVRing > kRefPasses, "the ring must hold the referenced passes and the one being written");
static_assert(kRecCap >= 128 && (kRecCap & (kRecCap - 1)) == 0, "record ring: >= 128 records, a power of two");

// Sample window of a pose: samples kx in [x0, x0 + nx), ky in [y0, y0 + ny); the LDS z-sample tile stores
// them row-major, sample (kx, ky) at (ky - y0) * nx + (kx - x0).
struct SampleWin {
    int x0, y0, nx, ny;
    // every vertex of the pose has 1 <= z < 2^41 and |x|, |y| < 2^41 after the projection (pose_window's bounds),
    // so the vertex pass needs no per-vertex range check of its unscaled division (see the vertex pass)
    int fastdiv;
    // the vertex stage may skip the projection's zero entries (raster_phase): a.proj_sparse, every model vertex
    // finite and the camera rows' bounds over the model's box far from FLT_MAX
    int sparse;
    // a fastdiv pose whose proven box of computed screen coordinates (pose_window) lies inside the image, [0, W-1] x
    // [0, H-1], and whose window none of pose_window's clamps to the sampled image has cut: the vertex pass needs no
    // clamp to the image (vertex_bounds), the fragment test's area reciprocal no scaling steps (pcore_fdiv.h,
    // recip_interior) and the triangle stage no clip to the whole window (raster_phase, WHOLE).  A property of the pose:
    // a chunk keeps its window's flag.
    int interior;
};

// IDPASS = false: depth pass (atomicMin of the fragment depth).  IDPASS = true: colour id pass over the
// final depths: the fragments whose depth equals the sample's minimum leave the lowest original triangle
// index -- the colour the reference's serial z-test (strict <) keeps.
// RZ: r.z0, r.z1, r.z2 hold the reciprocal depths v_rcp_f32(z) and exact_z(z0, z1, z2) fetches the depths for the
// lanes of the fragment depth's IEEE fallback (the depth pass of a fastdiv pose, raster_phase)
template <bool IDPASS = false, int BARY = 0, bool RZ = false, class ExactZ>
__device__ __forceinline__ void raster_sample(const TriRec& r, int kx, int ky, int s, int H, const SampleWin& w,
                                              int32_t* zbuf, int32_t* cid, uint32_t id, ExactZ&& exact_z) {
    const float P0 = (float)(kx * s);
    const float P1 = (float)(H - 1 - ky * s);
    int32_t d;
    bool in;
    if constexpr (RZ)
        in = fragment_rz<BARY>(r.a0, r.a1, r.b0, r.b1, r.c0, r.c1, r.z0, r.z1, r.z2, P0, P1, d, exact_z);
    else
        in = fragment<BARY>(r.a0, r.a1, r.b0, r.b1, r.c0, r.c1, r.z0, r.z1, r.z2, P0, P1, d, w.fastdiv != 0);
    // inside the window: (ky - y0) nx + (kx - x0), as one multiply-add of the sample's halves less the wave-uniform
    // y0 nx + x0 (ky and nx are below 2^24 and their product below 2^32, as in the product of (ky - y0) it replaces)
    const int k = (int)(__umul24((uint32_t)ky, (uint32_t)w.nx) + (uint32_t)kx) - (w.y0 * w.nx + w.x0);
    if constexpr (IDPASS) {
        if (in && d == zbuf[k]) atomicMin(&cid[k], (int32_t)id);
    } else {
        // only inside lanes take part: an outside lane's INT_MAX min changed nothing but still collided with the
        // inside lanes on the same bank (C2: SQ_LDS_BANK_CONFLICT 15.1 M -> 11.0 M per launch, time unchanged)
        if (in) atomicMin(&zbuf[k], d);
    }
}

size_t fused_lds_bytes(int tile_samples, int bitmap_words, bool colour) {
    auto al = [](size_t b) { return (b + 15) & ~size_t(15); };
    size_t b = al((size_t)tile_samples * 4);
    b += al((size_t)kWaves * kRingSlots * 8);
    b += al((size_t)kWaves * kRingSlots * 4);
    b += al((size_t)kWaves * 2 * kWave * 8);
    b += al((size_t)kWaves * kRecStride * 8);
    if (colour) b += al((size_t)kWaves * kRecStride * 4);
    b += al((size_t)bitmap_words * 4);
    b += 48;  // counters: [0] bad, [1] explained, [2] points; [4..10] the pose window (fused_cost_kernel)
    return b;
}

__device__ __forceinline__ FusedSmem carve_smem(unsigned char* smem_raw, int nsamp, int bitmap_words,
                                                bool colour = false) {
    auto al = [](size_t b) { return (b + 15) & ~size_t(15); };
    FusedSmem sm;
    unsigned char* p = smem_raw;
    sm.zbuf = (int32_t*)p; p += al((size_t)nsamp * 4);
    sm.vxy = (float2*)p; p += al((size_t)kWaves * kRingSlots * 8);
    sm.vz = (float*)p; p += al((size_t)kWaves * kRingSlots * 4);
    sm.vbd = (uint2*)p; p += al((size_t)kWaves * 2 * kWave * 8);
    sm.ring = (uint2*)p; p += al((size_t)kWaves * kRecStride * 8);
    sm.ring_id = nullptr;
    if (colour) { sm.ring_id = (uint32_t*)p; p += al((size_t)kWaves * kRecStride * 4); }
    sm.bitmap = (uint32_t*)p; p += al((size_t)bitmap_words * 4);
    sm.counters = (int32_t*)p;
    return sm;
}

template <int STRIDE>
__device__ __forceinline__ int floor_div(int v, int s) {
    if constexpr (STRIDE == 8) return v >> 3;  // arithmetic shift == floor division by 8
    else {
        const int q = v / s;
        return (v % s != 0 && v < 0) ? q - 1 : q;
    }
}

// Sample window of a triangle whose screen coordinates are not NaN (finite or infinite), from the reference's
// bounding box and loop bounds (image_renderer.cuh:86-111): bmin = max(0, min p), first pixel trunc(bmin + 0.5);
// bmax = min(W-1, max p), last pixel floor(bmax) -- for non-NaN inputs the ternary chains of bbox_ref() are exactly
// these min / max.  Clamping to [0, 65536] / [-65536, W-1] first changes no window of a <= 16384-pixel image and
// keeps the conversions in range.  Sample kx covers raster column kx * s, sample row ky raster row H-1-ky*s:
//   a0 = ceil(trunc(max(0, min x) + 0.5) / s)      a1 = floor(floor(min(W-1, max x)) / s)
//   b0 = ceil((H-1 - floor(min(H-1, max y))) / s)  b1 = floor((H-1 - trunc(max(0, min y) + 0.5)) / s)
// Each bound is a monotone function of the triangle's min or max coordinate, so it equals the min or max of that
// function over the three vertices: a0 = min A0(x_i), a1 = max A1(x_i), b0 = min B0(y_i), b1 = max B1(y_i), and
// clipping to the pose window commutes as well.  The vertex pass stores (A0, B0) and (A1, B1) as int16 pairs;
// the triangle stage takes two packed minima and two packed maxima.  At stride 8 every bound fits int16
// (|bound| <= (16384 + 65536) / 8); the generic stride clamps them to +-32767, which leaves a window of a
// <= 16384-sample image empty exactly when it was.  A NaN screen coordinate marks the vertex with -32768 lower
// bounds (a real lower bound is >= 0), and its triangles take the reference's NaN-propagating bbox instead.
// floor(v + 0.5) and floor(v) of a finite float of magnitude < 2^23 (exact), one instruction each
__device__ __forceinline__ int cvt_rpi(float v) {
    int r;
    asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}
__device__ __forceinline__ int cvt_flr(float v) {
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}

typedef short short2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ short2v as_s2(uint32_t v) { return __builtin_bit_cast(short2v, v); }
constexpr uint32_t kNanBounds = 0x80008000u;

// INTERIOR: the vertex of an interior pose (SampleWin::interior), without the four clamps.  pose_window proves
// 0 <= xlo <= sx <= xhi <= W-1 = cmax0 for the computed sx of every vertex, so v_med3(sx, 0, 65536) = sx (0 <= sx <=
// 16383 < 65536) and v_med3(sx, -65536, cmax0) = sx (-65536 < sx <= cmax0); the same for sy with H-1 = cmax1.  (A sum
// sx = t + W/2 that is zero is +0 under round-to-nearest, and both conversions take either zero to 0.)
template <int STRIDE, bool INTERIOR = false>
__device__ __forceinline__ uint2 vertex_bounds(float sx, float sy, int s, float cmax0, float cmax1, int H,
                                              bool finite = false) {
    if (!finite && __builtin_isunordered(sx, sy)) return make_uint2(kNanBounds, 0u);
    const int ss = STRIDE > 0 ? STRIDE : s;
    // sx, sy are not NaN here, so each clamp is one v_med3_f32, and the clamped values are small enough
    // (|v| <= 65536 < 2^23) that v + 0.5 is exact: trunc(v + 0.5) = floor(v + 0.5) for v >= 0 is one
    // v_cvt_rpi_i32_f32, floor(v) one v_cvt_flr_i32_f32 (cvt_rpi / cvt_flr below)
    int lo0, lo1, hi0, hi1;
    if constexpr (INTERIOR) {
        lo0 = cvt_rpi(sx);
        lo1 = cvt_rpi(sy);
        hi0 = cvt_flr(sx);
        hi1 = cvt_flr(sy);
        if constexpr (STRIDE == 8) {
            // The two words built in place and shifted as int16 pairs:
            //   (A0, B0) = (lo0 + 7, H + 6 - hi1) >> 3      (A1, B1) = (hi0, H - 1 - lo1) >> 3
            // The four converted values lie in [0, 16383] (sx in [0, W-1], sy in [0, H-1], W, H <= 16384), so every
            // half lies in [0, H + 6], inside int16: each is the 32-bit expression of the scalar form bit for bit (H - 1
            // - hi1 + 7 = H + 6 - hi1; a shift of a non-negative value).  The subtractions write the upper half of the
            // word that already holds the lower one (SDWA, the rest of the destination preserved), and one packed shift
            // per word divides both halves: five instructions for the nine of the scalar form (packing with
            // v_cvt_pk_i16_i32 and a packed multiply-add by (1, -1) took eight: gfx9 reads one scalar constant per
            // instruction).  A VALU write through dst_sel or of a packed result needs one wait state before a VALU
            // instruction reads the register (the compiler does not see into the asm): the order below and the closing
            // s_nop give it to both words.
            uint32_t p0 = (uint32_t)(lo0 + 7), p1 = (uint32_t)hi0;
            asm("v_sub_u32_sdwa %0, %2, %3 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
                "v_sub_u32_sdwa %1, %4, %5 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
                "v_pk_ashrrev_i16 %0, 3, %0 op_sel_hi:[0,1]\n\t"
                "v_pk_ashrrev_i16 %1, 3, %1 op_sel_hi:[0,1]\n\t"
                "s_nop 0"  // the same wait state after the last packed write, whatever the compiler puts next
                : "+v"(p0), "+v"(p1)
                : "s"(H + 6), "v"(hi1), "s"(H - 1), "v"(lo1));
            return make_uint2(p0, p1);
        }
    } else {
        lo0 = cvt_rpi(__builtin_amdgcn_fmed3f(sx, 0.0f, 65536.0f));
        lo1 = cvt_rpi(__builtin_amdgcn_fmed3f(sy, 0.0f, 65536.0f));
        hi0 = cvt_flr(__builtin_amdgcn_fmed3f(sx, -65536.0f, cmax0));
        hi1 = cvt_flr(__builtin_amdgcn_fmed3f(sy, -65536.0f, cmax1));
    }
    int A0 = floor_div<STRIDE>(lo0 + ss - 1, s), A1 = floor_div<STRIDE>(hi0, s);
    int B0 = floor_div<STRIDE>(H - 1 - hi1 + ss - 1, s), B1 = floor_div<STRIDE>(H - 1 - lo1, s);
    if constexpr (STRIDE == 0) {
        A0 = min(A0, 32767);
        B0 = min(B0, 32767);
        A1 = max(A1, -32767);
        B1 = max(B1, -32767);
    }
    return make_uint2(((uint32_t)A0 & 0xffffu) | ((uint32_t)B0 << 16), ((uint32_t)A1 & 0xffffu) | ((uint32_t)B1 << 16));
}


// FD: the pose's class known at compile time (0: general, 1: fastdiv, 2: fastdiv and interior; the depth pass
// instantiates the three and picks one per pose, so a fastdiv pose's steps carry no NaN-triangle test or range checks at
// all, and an interior pose's no clamp of its vertices to the image and no scaling steps in the area's reciprocal), or
// -1 to read the fastdiv flag from the window (the colour id pass: the general fragment test and clamps)
//
// WHOLE: sw_in is the pose's own window, not a chunk of it (the un-chunked copy of fused_pose / render_cloud_kernel).
// With FD = 2 the triangle stage then does not clip the triangle's window to sw.  pose_window proves a box [xlo, xhi] x
// [ylo, yhi] that holds every vertex's computed sx, sy, and an interior pose's window is, unclamped (pose_window grants
// the class only then), [X0, X1] x [Y0, Y1] = [floor((xlo-1)/s), floor(xhi/s)] x [floor((H-1-yhi)/s), floor((H-ylo)/s)].
// The bounds of a vertex (vertex_bounds) are A0 = ceil(rpi(sx)/s) >= (sx - 0.5)/s > (xlo - 1)/s, A1 = floor(floor(sx)/s)
// <= sx/s <= xhi/s, B0 = ceil((H-1-floor(sy))/s) >= (H-1-yhi)/s and B1 = floor((H-1-rpi(sy))/s) <= (H-0.5-sy)/s <
// (H-ylo)/s: integers, so X0 <= A0, A1 <= X1, Y0 <= B0, B1 <= Y1 for every vertex (the float quotients of pose_window
// round monotonically and an integer is its own rounding, so the computed floors keep the inequalities).  A triangle's lo
// is a minimum of (A0, B0) and its hi a maximum of (A1, B1) over three vertices, so max(lo, first) = lo and min(hi, last)
// = hi in both halves whether the window is empty or not: the clip changes no bit of lo, hi or d.  A chunk is a proper
// part of the window and keeps the clip.
template <int STRIDE, bool IDPASS = false, int FD = -1, bool WHOLE = false>
__device__ __forceinline__ void raster_phase(const FusedArgs& a, const FusedSmem& sm, int pose, const SampleWin& sw_in,
                                             int32_t* cid, FProf& fp) {
    SampleWin sw = sw_in;
    if constexpr (FD >= 0) sw.fastdiv = FD >= 1;
    constexpr bool kNoClip = WHOLE && FD == 2 && !IDPASS;
    // the fragment test without its halves: the depth pass of a fastdiv pose only; with the unscaled area reciprocal:
    // of an interior pose only (pcore_fdiv.h)
    constexpr int kBary = IDPASS || FD < 1 ? 0 : FD;
    constexpr bool kInterior = FD == 2 && !IDPASS;
    // The vertex ring keeps v_rcp_f32(z) instead of z: the depth pass of a fastdiv pose.  There the fragment test uses a
    // vertex depth only as v_rcp_f32(z) -- which the vertex pass issues anyway, as the first step of its refined
    // reciprocal -- except in the certified depth's rare IEEE fallback, whose lanes compute z again from the stream
    // (ring_z below).
    constexpr bool kRz = FD >= 1 && !IDPASS;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: scalar loads of stream headers
    const int lane = tid & 63;
    const int s = STRIDE > 0 ? STRIDE : a.stride;
    const int W = a.width, H = a.height;
    // pose (wave-uniform -> scalar loads)
    const float* P = a.poses + (size_t)16 * pose;
    const float m00 = P[0], m01 = P[1], m02 = P[2], m03 = P[3];
    const float m10 = P[4], m11 = P[5], m12 = P[6], m13 = P[7];
    const float m20 = P[8], m21 = P[9], m22 = P[10], m23 = P[11];
    const int model = a.pose_model[pose];
    // Projection with compute_proj's zeros skipped: the reference's ((p00 x + p01 y) + p02 z) + p03 with
    // p01 = p03 = 0 differs from p00 x + p02 z only in the sign of a zero result -- which x / z * W/2 + W/2
    // does not see (both give W/2 exactly) -- as long as the skipped products 0 * y are zeros, i.e. the camera
    // point is finite.  It is when every model vertex is finite (model_box flag) and the bound of |row . v|
    // over the model's box (B below, as in pose_window) stays far from FLT_MAX; NaN entries fail the test.
    // The test is pose_window's (SampleWin::sparse), made once per workgroup with the window.
    const bool proj_sparse = sw.sparse != 0;
    __syncthreads();

    // ---------------- phase 1: raster of the sampled pixels ----------------
    const float Wf = (float)W, Hf = (float)H;
    const float hw = Wf / 2.0f, hh = Hf / 2.0f;
    const float cmax0 = (float)(W - 1), cmax1 = (float)(H - 1);
    float2* vxy = sm.vxy + wave * kRingSlots;
    float* vz = sm.vz + wave * kRingSlots;
    uint2* vbd = sm.vbd + wave * 2 * kWave;
    // the pose window as int16 pairs (first sample, last sample); an empty window has last < first
    const short2v wfirst = {(short)sw.x0, (short)sw.y0};
    const short2v wlast = {(short)(sw.x0 + sw.nx - 1), (short)(sw.y0 + sw.ny - 1)};
    // The ring as 32-bit words behind one opaque LDS byte address in an SGPR: the compiler otherwise keeps the
    // workgroup's LDS base and adds the ring's constant offset to every record address in a VALU instruction.
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    uint32_t ring_addr = (uint32_t)(uintptr_t)(lds_u32*)reinterpret_cast<uint32_t*>(sm.ring + wave * kRecStride);
    asm("" : "+s"(ring_addr));
    lds_u32* const ring = (lds_u32*)(uintptr_t)ring_addr;
    auto ring_put = [ring](int slot, uint32_t x, uint32_t y) { ring[2 * slot] = x; ring[2 * slot + 1] = y; };
    auto ring_get = [ring](int slot) { return make_uint2(ring[2 * slot], ring[2 * slot + 1]); };
    uint32_t* ring_id = IDPASS ? sm.ring_id + wave * kRecStride : nullptr;
    // record ring: wave-uniform monotone counters of appended and flushed records; record i lives in slot
    // i mod kRecCap.  Full 64-record batches are flushed as soon as they exist; a partial batch only when a
    // vertex pass would overwrite vertices a pending record may reference, at a stream switch and at the end.
    int rec_total = 0, rec_done = 0;
    // kRz: the stream whose vertices the ring holds -- its first vertex pass and how many of its passes are written.
    // Set after the flush at a stream switch (which still serves the previous stream's records) and kept past the last
    // stream for the final flush.
    int ring_first = 0, ring_passes = 0;
    // The camera z of the vertex in a ring slot (buffer * 64 + lane), for the fallback lanes.
    // A pending record's slot has not been overwritten (the flush rules of the ring), so it holds the latest written
    // pass p of the stream with p mod kVRing == buffer; that pass is sverts[(ring_first + p) * 64 ..], and z is the
    // vertex pass's own row4 on it (contraction off: the same bits).  0 <= p < ring_passes, so the read lies within
    // the passes this wave has already loaded from its stream, [ring_first, ring_first + ring_passes) * 64; the clamp to
    // pass 0 keeps it there even for a slot no pass has written, which no record names.
    auto ring_z = [&](uint32_t slot) {
        const int last = ring_passes - 1, d = last - (int)(slot >> 6);
        const int p = d >= 0 ? last - d % kVRing : 0;
        const float* v = reinterpret_cast<const float*>(a.sverts + (size_t)(ring_first + p) * kStepSlots + (slot & 63u));
        return row4(m20, m21, m22, m23, v[0], v[1], v[2]);
    };

    const int dbg = dbg_skip_bits(a);  // the ablation mask: the constant 0 in the production build
    FlushStats fs;
    auto flush = [&](int count) {  // the `count` oldest pending records
        fp.mark(2);
        wave_sync();
        if (!(dbg & 1)) {
            for (int base = 0; base < count; base += kWave) {
                fs.batch(lane, min(count - base, kWave));
                if (base + lane < count) {
                    const int j = (rec_done + base + lane) & (kRecCap - 1);
                    const uint2 rec = ring_get(j);
                    const uint32_t id = IDPASS ? ring_id[j] : 0u;
                    const int i0 = rec.x & 511, i1 = (rec.x >> 9) & 511, i2 = (rec.x >> 18) & 511;
                    const float2 q0 = vxy[i0], q1 = vxy[i1], q2 = vxy[i2];
                    TriRec r;
                    r.a0 = q0.x; r.a1 = q0.y;
                    r.b0 = q1.x; r.b1 = q1.y;
                    r.c0 = q2.x; r.c1 = q2.y;
                    r.z0 = vz[i0]; r.z1 = vz[i1]; r.z2 = vz[i2];
                    // the depths are needed only past the inside test, but reading them with the screen
                    // coordinates puts all six reads in one LDS round trip instead of two
                    asm volatile("" : "+v"(r.z0), "+v"(r.z1), "+v"(r.z2));
                    // one record per (triangle, sample): the sample is rec.y = kx | ky << 16
                    fs.record();
                    raster_sample<IDPASS, kBary, kRz>(r, (int)(rec.y & 0xffffu), (int)(rec.y >> 16), s, H, sw, sm.zbuf,
                                                      cid, id, [&](float& z0, float& z1, float& z2) {
                                                          z0 = ring_z(rec.x & 511u);
                                                          z1 = ring_z((rec.x >> 9) & 511u);
                                                          z2 = ring_z((rec.x >> 18) & 511u);
                                                      });
                }
            }
        }
        rec_done += count;
        wave_sync();
        fp.mark(3);
    };

    if (model < 0 || model >= a.num_models) return;
    const int st_lo = a.model_st_lo[model], st_hi = a.model_st_hi[model];
    fp.mark(0);
    for (int st = st_lo + wave; st < st_hi; st += kWaves) {
        const int4 sd = a.streams[st];  // first step, end step, first vertex pass, end vertex pass
        if (rec_total > rec_done) {      // a new stream numbers its ring slots from buffer 0
            fs.partial_flush(lane);
            flush(rec_total - rec_done);
        }
        ring_first = sd.z;
        ring_passes = 0;
        // hist[k]: rec_total when pass P-1-k was written (P = the next pass).  A batch issued after pass h
        // references passes >= h - kRefPasses + 1, so before pass P overwrites the buffer of pass P - kVRing every
        // record appended before pass P - (kVRing - kRefPasses) was written must be flushed.
        int hist[kVRing - kRefPasses];
#pragma unroll
        for (int k = 0; k < kVRing - kRefPasses; k++) hist[k] = rec_total;
        int buf = 0;                 // ring buffer of the next vertex pass
        // wave-uniform stream pointers (SGPRs): the current step's triangle slots and the next unconsumed vertex pass
        const uint32_t* tp = a.stris + (size_t)sd.x * kStepSlots;
        const uint32_t* op = IDPASS ? a.stri_orig + (size_t)sd.x * kStepSlots : nullptr;
        const float4* vq = a.sverts + (size_t)sd.z * kStepSlots;
        // one step: the current step's triangle slots / vertex pass in (cv, ct, cidt); prefetches the next step's
        // triangle slots and the next unconsumed vertex pass into (ncv, nct, ncid) -- unconditional loads (after a
        // stream's last step they read the next stream's first, or the padding step and pass the upload appends).
        // The loop below alternates two register sets, so no copy of a prefetched register makes the wave wait
        // for the load at the end of its step.
        auto run_step = [&](int step, const float4& cv, const uint32_t ct, const uint32_t cidt, float4& ncv,
                            uint32_t& nct, uint32_t& ncid) {
            (void)step;
            tp += kStepSlots;
            nct = tp[lane];
            if constexpr (IDPASS) {
                op += kStepSlots;
                ncid = op[lane];
            } else {
                ncid = 0u;
            }
            // the step's "vertex pass first" flag is in every triangle slot (pcore_internal.h)
            const bool vpass = (__builtin_amdgcn_readfirstlane((int)ct) >> 30) & 1;
            if (vpass) vq += kStepSlots;
            ncv = vq[lane];
            if (vpass) {
                if (rec_done < hist[kVRing - kRefPasses - 1]) {
                    fs.partial_flush(lane);
                    flush(rec_total - rec_done);
                }
                // vertex stage: model transform, keep camera z, projection rows 0/1, viewport
                // (image_renderer.cuh:296-305, 82-84)
                // every lane transforms its slot: a padding lane (cv.w == 0) writes a slot no triangle names
                if (!(dbg & 8)) {
                    const float lx = row4(m00, m01, m02, m03, cv.x, cv.y, cv.z);
                    const float ly = row4(m10, m11, m12, m13, cv.x, cv.y, cv.z);
                    const float lz = row4(m20, m21, m22, m23, cv.x, cv.y, cv.z);
                    float px, py;
                    if (proj_sparse) {
                        px = a.p00 * lx + a.p02 * lz;
                        py = a.p11 * ly + a.p12 * lz;
                    } else {
                        px = row4(a.p00, a.p01, a.p02, a.p03, lx, ly, lz);
                        py = row4(a.p10, a.p11, a.p12, a.p13, lx, ly, lz);
                    }
                    // px / lz and py / lz sharing one refined reciprocal of lz, IEEE-exact where every exponent is
                    // in range (pcore_fdiv.h); there |q| < 2^81, so (q * W) / 2 is q * (W / 2) exactly (a power-of-
                    // two scaling, no overflow or underflow).  Elsewhere the reference's expressions.  With the pose's
                    // fastdiv bound (1 <= lz < 2^41, |px|, |py| < 2^41) the only operand out of range is a numerator
                    // below 2^-40, whose quotient (IEEE or unscaled) is below 2^-40: q * W/2 + W/2 rounds to W/2 either
                    // way, so no per-vertex check is needed.
                    float r0;  // v_rcp_f32(lz)
                    const float r1 = recip_refined(lz, r0);
                    float qx = quot_refined(px, lz, r1), qy = quot_refined(py, lz, r1);
                    float sx = qx * hw + hw, sy = qy * hh + hh;
                    if (!sw.fastdiv) {
                        const uint32_t ex = fexp_bits(px), ey = fexp_bits(py), ez = fexp_bits(lz);
                        if (!fdiv_range_ok(min(min(ex, ey), ez), max(max(ex, ey), ez))) {
                            asm volatile("");
                            qx = px / lz;
                            qy = py / lz;
                            sx = qx * Wf / 2.0f + Wf / 2.0f;
                            sy = qy * Hf / 2.0f + Hf / 2.0f;
                        }
                    }
                    vxy[buf * kWave + lane] = make_float2(sx, sy);
                    vz[buf * kWave + lane] = kRz ? r0 : lz;
                    // a wave-uniform branch, so a fastdiv pose's pass carries no NaN test, default bounds or exec
                    // masking (the screen coordinates are finite there)
                    uint2 vb;
                    if constexpr (kInterior) vb = vertex_bounds<STRIDE, true>(sx, sy, s, cmax0, cmax1, H, true);
                    else if (sw.fastdiv) vb = vertex_bounds<STRIDE>(sx, sy, s, cmax0, cmax1, H, true);
                    else vb = vertex_bounds<STRIDE>(sx, sy, s, cmax0, cmax1, H, false);
                    vbd[(buf & 1) * kWave + lane] = vb;
                }
#pragma unroll
                for (int k = kVRing - kRefPasses - 1; k > 0; k--) hist[k] = hist[k - 1];
                hist[0] = rec_total;
                buf = buf + 1 == kVRing ? 0 : buf + 1;
                ring_passes++;
                fs.vertex_pass(lane);
                wave_sync();
            }
            fp.mark(1);
            if (!(dbg & 2)) {
                // the triangle's clipped window, packed: pos = first sample (kx0 | ky0 << 16), dbits = its size less
                // one, (nx - 1) | (ny - 1) << 16
                uint32_t pos = 0u, dbits = 0u;
                bool nonempty;
                // bt: the ballot of nonempty; brest: of the lanes that need the general code -- a non-empty window
                // of more than one sample (d != 0), or a NaN vertex, whose window is not d
                uint64_t bt, brest;
                // the vertices' ring slots (9 bits each) and, for the bounds, their pass parity + lane (7 bits);
                // the slots proper are decoded only where a rare path needs the screen coordinates
                auto slot_of = [ct](int k) { return (int)((ct >> (9 * k)) & 511u); };
                // a padding slot names slot 0 three times: its bounds are read (harmless) and its window counts as empty
                const bool pad = ct >> 31;
                bool nan_tri = false;
                {
                    // bit-field extracts as v_bfe (asm: the compiler turns them back into shift / mask / add, three
                    // instructions per address instead of v_bfe + v_lshl_add)
                    uint32_t i1, i2;
                    asm("v_bfe_u32 %0, %1, 9, 7" : "=v"(i1) : "v"(ct));
                    asm("v_bfe_u32 %0, %1, 18, 7" : "=v"(i2) : "v"(ct));
                    const uint2 w0 = vbd[ct & 127u], w1 = vbd[i1], w2 = vbd[i2];
                    short2v lo = __builtin_elementwise_min(__builtin_elementwise_min(as_s2(w0.x), as_s2(w1.x)), as_s2(w2.x));
                    short2v hi = __builtin_elementwise_max(__builtin_elementwise_max(as_s2(w0.y), as_s2(w1.y)), as_s2(w2.y));
                    // (fastdiv poses have finite screen coordinates: no NaN vertex)
                    if (!sw.fastdiv) nan_tri = lo.x < 0 && !pad;
                    if constexpr (!kNoClip) {  // (the whole window of an interior pose holds lo and hi: WHOLE above)
                        lo = __builtin_elementwise_max(lo, wfirst);
                        hi = __builtin_elementwise_min(hi, wlast);
                    }
                    const short2v d = hi - lo;  // (nx - 1, ny - 1), negative where the window is empty
                    pos = __builtin_bit_cast(uint32_t, lo);
                    dbits = __builtin_bit_cast(uint32_t, d);
                    nonempty = (dbits & 0x80008000u) == 0u && !pad;
                    // the wave masks are combined from the ballots of the plain compares with scalar instructions
                    // (a ballot of the combined predicate costs two more VALU instructions)
                    bt = __ballot((dbits & 0x80008000u) == 0u) & __ballot(!pad);
                    brest = bt & __ballot(dbits != 0u);
                    if (!sw.fastdiv) brest |= __ballot(nan_tri);
                }
                // One-sample fast path: when no lane of the step needs the general code, every non-empty window is
                // exactly one sample (d == 0 in both halves) -- as in every step of a mesh whose triangles span less
                // than the sample stride -- and the record queue below takes the non-empty lanes as they are: qd =
                // nonempty, the record (ct, pos), with no sample count, size or big-triangle ballot.  A step with any
                // other lane takes the general code for all its lanes.  The records of a step, their order included,
                // are the ones the general code alone would queue, so every z-sample, cloud, colour id and cost keeps
                // its bits; the ring rules are unchanged: an append adds at most 64 records to fewer than 64 pending
                // and full batches are flushed right after it, and rec_total advances by the step's total before the
                // next vertex pass reads hist[].  Both kinds of step share the queue and its flush: a second inlined
                // copy of the flush grew the kernel's code by 13 % and cost time where windows are large.
                fs.step(lane, brest ? 0ull : bt, brest, ct);
                // nxy = the window's size (nx | ny << 16), nk = nx * ny samples (0: none); general steps only
                uint32_t nxy = 0u;
                int nk = 0;
                bool qd = nonempty;  // the lanes that queue their first sample
                uint64_t bq = bt;
                if (brest) {
                    const short2v one = {1, 1};
                    nxy = __builtin_bit_cast(uint32_t, as_s2(dbits) + one);
                    nk = nonempty ? (int)__umul24(nxy & 0xffffu, nxy >> 16) : 0;
                    if (nan_tri) {
                        // NaN screen coordinates: the reference's exact bbox with its NaN-propagating clamps
                        const float2 q0 = vxy[slot_of(0)], q1 = vxy[slot_of(1)], q2 = vxy[slot_of(2)];
                        const float p[3][2] = {{q0.x, q0.y}, {q1.x, q1.y}, {q2.x, q2.y}};
                        float bmin[2], bmax[2];
                        bbox_ref(p, cmax0, cmax1, bmin, bmax);
                        int kx0 = 0, ky0 = 0, nx = 0, ny = 0;
                        nk = sample_window<STRIDE>(bmin, bmax, s, H, kx0, ky0, nx, ny);
                        if (nk > 0) {  // clip to the pose window
                            const int kx1 = min(kx0 + nx, sw.x0 + sw.nx), ky1 = min(ky0 + ny, sw.y0 + sw.ny);
                            kx0 = max(kx0, sw.x0);
                            ky0 = max(ky0, sw.y0);
                            nx = kx1 - kx0;
                            ny = ky1 - ky0;
                            nk = (nx > 0 && ny > 0) ? nx * ny : 0;
                        }
                        pos = (uint32_t)kx0 | ((uint32_t)ky0 << 16);
                        nxy = (uint32_t)nx | ((uint32_t)ny << 16);
                    }
                    // large triangles: whole-wave cooperative
                    uint64_t big = __ballot(nk > kSmallK);
                    fs.slow_step(lane, big, nk);
                    if (big) {
                        // the big triangles' screen vertices, read again (rare: not kept in registers through the step)
                        float2 q0 = make_float2(0.f, 0.f), q1 = q0, q2 = q0;
                        float z0 = 0.0f, z1 = 0.0f, z2 = 0.0f;
                        if (nk > kSmallK) {
                            const int i0 = slot_of(0), i1 = slot_of(1), i2 = slot_of(2);
                            q0 = vxy[i0];
                            q1 = vxy[i1];
                            q2 = vxy[i2];
                            z0 = vz[i0];
                            z1 = vz[i1];
                            z2 = vz[i2];
                        }
                        do {
                            const int j = __ffsll((unsigned long long)big) - 1;
                            big &= big - 1;
                            // j is wave-uniform: v_readlane into SGPRs (no LDS round trip)
                            auto rl = [&](float x) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j)); };
                            TriRec rb;
                            rb.a0 = rl(q0.x); rb.a1 = rl(q0.y);
                            rb.b0 = rl(q1.x); rb.b1 = rl(q1.y);
                            rb.c0 = rl(q2.x); rb.c1 = rl(q2.y);
                            rb.z0 = rl(z0); rb.z1 = rl(z1); rb.z2 = rl(z2);
                            const uint32_t bpos = (uint32_t)__builtin_amdgcn_readlane((int)pos, j);
                            const int bkx0 = (int)(bpos & 0xffffu), bky0 = (int)(bpos >> 16);
                            const int bnx = (int)((uint32_t)__builtin_amdgcn_readlane((int)nxy, j) & 0xffffu);
                            const int bnk = __builtin_amdgcn_readlane(nk, j);
                            const uint32_t bid = IDPASS ? (uint32_t)__builtin_amdgcn_readlane((int)cidt, j) : 0u;
                            const uint32_t bct = kRz ? (uint32_t)__builtin_amdgcn_readlane((int)ct, j) : 0u;
                            // q / bnx without an integer division: the float quotient is within 1e-3 of q / bnx (q / bnx
                            // is at most the sample rows), so one correction step gives the exact row
                            const float inv_nx = 1.0f / (float)bnx;
                            for (int q = lane; q < bnk; q += kWave) {
                                int iy = (int)(((float)q + 0.5f) * inv_nx), ix = q - iy * bnx;
                                if (ix < 0) { iy--; ix += bnx; } else if (ix >= bnx) { iy++; ix -= bnx; }
                                raster_sample<IDPASS, kBary, kRz>(rb, bkx0 + ix, bky0 + iy, s, H, sw, sm.zbuf, cid, bid,
                                                                  [&](float& z0, float& z1, float& z2) {
                                                                      z0 = ring_z(bct & 511u);
                                                                      z1 = ring_z((bct >> 9) & 511u);
                                                                      z2 = ring_z((bct >> 18) & 511u);
                                                                  });
                            }
                        } while (big);
                    }
                    qd = nk > 0 && nk <= kSmallK;
                    bq = __ballot(qd);
                }
                // small triangles: one record per (triangle, sample) into the wave's record ring -- the first
                // sample of every queued triangle, then (general steps) the second to fourth of those touching more,
                // one ballot round each; full 64-record batches are flushed after every round (<= 127 pending)
                if (qd) {  // the record keeps the whole triangle slot word (the flush reads its 27 slot bits)
                    const int slot = (rec_total + mbcnt64(bq)) & (kRecCap - 1);
                    ring_put(slot, ct, pos);
                    if (IDPASS) ring_id[slot] = cidt;
                }
                rec_total += __popcll(bq);
                while (rec_total - rec_done >= kWave) flush(kWave);  // full batches only
                if (brest && __ballot(qd && nk > 1)) {
                    for (int q = 1; q < kSmallK; q++) {
                        const bool qr = qd && nk > q;
                        const uint64_t br = __ballot(qr);
                        if (!br) break;
                        if (qr) {  // sample q of the window, row-major (nx * ny <= 4)
                            const int nx = (int)(nxy & 0xffffu);
                            const int iy = nx == 1 ? q : (nx == 2 ? q >> 1 : 0), ix = q - iy * nx;
                            const int slot = (rec_total + mbcnt64(br)) & (kRecCap - 1);
                            ring_put(slot, ct, pos + (uint32_t)ix + ((uint32_t)iy << 16));
                            if (IDPASS) ring_id[slot] = cidt;
                        }
                        rec_total += __popcll(br);
                        while (rec_total - rec_done >= kWave) flush(kWave);
                    }
                }
            }
            fp.mark(2);
        };
        float4 cvA = vq[lane], cvB;
        uint32_t ctA = tp[lane], ctB, cidA, cidB;
        cidA = IDPASS ? op[lane] : 0u;
        for (int step = sd.x; step < sd.y; step += 2) {
            run_step(step, cvA, ctA, cidA, cvB, ctB, cidB);
            if (step + 1 < sd.y) run_step(step + 1, cvB, ctB, cidB, cvA, ctA, cidA);
        }
    }
    if (rec_total > rec_done) flush(rec_total - rec_done);
}

// Conservative sample window of a pose ("Pose windows").  Lanes 0-7 of every wave project the
// corners of the model's bounding box with the vertex stage's own arithmetic; the window is their screen
// box widened by a bound on the float error of any vertex's projection, mapped to samples through the
// bounds of vertex_window (every triangle window lies inside).  The whole sampled image when the box is
// not finite or comes within 5 % of its depth magnitude of the camera plane.  Wave-uniform; every wave of
// the workgroup computes the same window.
// Always inline: a call would make the kernel keep its argument block in scratch memory to pass the reference.
__device__ __forceinline__ SampleWin pose_window(const FusedArgs& a, int model, const float (&m)[12], int s) {
    const float4 lo = a.model_box[2 * model], hi = a.model_box[2 * model + 1];
    // magnitude of the terms of each camera row over the box (bounds the rounding of any vertex's row)
    const float ax = fmaxf(fabsf(lo.x), fabsf(hi.x)), ay = fmaxf(fabsf(lo.y), fabsf(hi.y));
    const float az = fmaxf(fabsf(lo.z), fabsf(hi.z));
    const float Bx = fabsf(m[0]) * ax + fabsf(m[1]) * ay + fabsf(m[2]) * az + fabsf(m[3]);
    const float By = fabsf(m[4]) * ax + fabsf(m[5]) * ay + fabsf(m[6]) * az + fabsf(m[7]);
    const float Bz = fabsf(m[8]) * ax + fabsf(m[9]) * ay + fabsf(m[10]) * az + fabsf(m[11]);
    const int sparse = (a.proj_sparse && lo.w != 0.0f && Bx < 1.0e30f && By < 1.0e30f) ? 1 : 0;  // NaN bounds fail
    const SampleWin whole = {0, 0, a.ws, a.hs, 0, sparse, 0};
    const int c = lane_id() & 7;
    const float x = (c & 1) ? hi.x : lo.x, y = (c & 2) ? hi.y : lo.y, z = (c & 4) ? hi.z : lo.z;
    const float Wf = (float)a.width, Hf = (float)a.height;
    const float lx = row4(m[0], m[1], m[2], m[3], x, y, z);
    const float ly = row4(m[4], m[5], m[6], m[7], x, y, z);
    const float lz = row4(m[8], m[9], m[10], m[11], x, y, z);
    const float px = row4(a.p00, a.p01, a.p02, a.p03, lx, ly, lz);
    const float py = row4(a.p10, a.p11, a.p12, a.p13, lx, ly, lz);
    const float sx = px / lz * Wf / 2.0f + Wf / 2.0f;
    const float sy = py / lz * Hf / 2.0f + Hf / 2.0f;
    const bool bad = !(fabsf(sx) < 1.0e7f) || !(fabsf(sy) < 1.0e7f) || !(lz > 0.0f);  // also NaN
    float lzmin = lz, sx0 = sx, sx1 = sx, sy0 = sy, sy1 = sy;
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {
        lzmin = fminf(lzmin, __shfl_xor(lzmin, off));
        sx0 = fminf(sx0, __shfl_xor(sx0, off));
        sx1 = fmaxf(sx1, __shfl_xor(sx1, off));
        sy0 = fminf(sy0, __shfl_xor(sy0, off));
        sy1 = fmaxf(sy1, __shfl_xor(sy1, off));
    }
    auto uni = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    lzmin = uni(lzmin); sx0 = uni(sx0); sx1 = uni(sx1); sy0 = uni(sy0); sy1 = uni(sy1);
    if ((__ballot(bad) & 0xffull) || lo.w == 0.0f) return whole;
    if (!(lzmin > 0.05f * Bz)) return whole;
    // |error of sx| <= (W/2) (Pbx / lzmin) eps (8 + 4 Bz / lzmin) + 4 eps (|sx| + W), Bz / lzmin <= 20
    const float eps = 5.9604645e-8f;
    const float Pbx = fabsf(a.p00) * Bx + fabsf(a.p01) * By + fabsf(a.p02) * Bz + fabsf(a.p03);
    const float Pby = fabsf(a.p10) * Bx + fabsf(a.p11) * By + fabsf(a.p12) * Bz + fabsf(a.p13);
    const float mgx = 2.0f + 256.0f * eps * (0.5f * Wf) * Pbx / lzmin + 8.0f * eps * (fmaxf(fabsf(sx0), fabsf(sx1)) + Wf);
    const float mgy = 2.0f + 256.0f * eps * (0.5f * Hf) * Pby / lzmin + 8.0f * eps * (fmaxf(fabsf(sy0), fabsf(sy1)) + Hf);
    if (!(mgx < 1.0e6f) || !(mgy < 1.0e6f)) return whole;
    const float xlo = sx0 - mgx, xhi = sx1 + mgx, ylo = sy0 - mgy, yhi = sy1 + mgy;
    // vertex_window: lo.x >= (sx - 0.5) / s, hi.x <= sx / s; lo.y >= (H - 1 - sy) / s, hi.y <= (H - 0.5 - sy) / s
    const float sf = (float)s;
    const int X0u = (int)floorf((xlo - 1.0f) / sf), X1u = (int)floorf(xhi / sf);
    const int Y0u = (int)floorf((Hf - 1.0f - yhi) / sf), Y1u = (int)floorf((Hf - ylo) / sf);
    const int X0 = max(0, X0u), X1 = min(a.ws - 1, X1u), Y0 = max(0, Y0u), Y1 = min(a.hs - 1, Y1u);
    // Every vertex's computed z is at least the corners' minimum less the rounding of two dot products
    // (<= 6 eps Bz); the margin 1e-5 Bz covers that.  |x|, |y| after the projection are below Pbx, Pby.
    // (The fragment test of a fastdiv pose relies on these bounds too: pcore_fdiv.h, frag_barycentrics.)
    const bool fastdiv = lzmin - 1.0e-5f * Bz >= 1.0f && Bz < 0x1p40f && Pbx < 0x1p40f && Pby < 0x1p40f;
    // interior: the box [xlo, xhi] x [ylo, yhi] holds every vertex's computed screen coordinates (it is what the window
    // above is made from) and lies inside the image; NaN bounds fail.  And none of the four clamps of the window to the
    // sampled image binds, so the window is the box's own and holds every triangle's window unclipped (raster_phase,
    // WHOLE).  With ws = W / s and hs = ceil(H / s) the first clamp binds where xlo < 1 and the last where s divides H and
    // H - ylo rounds to H; with any other ws, hs more would: such a pose is fastdiv only.  (With those ws, hs the two
    // clamps never cut a triangle's window -- A0 >= 0 and B1 <= (H - 1) / s = hs - 1 whatever the box -- so the test
    // buys a proof that does not lean on how the host derives ws and hs, not correctness.)
    const bool unclamped = X0u >= 0 && X1u <= a.ws - 1 && Y0u >= 0 && Y1u <= a.hs - 1;
    const bool interior = fastdiv && unclamped && xlo >= 0.0f && xhi <= Wf - 1.0f && ylo >= 0.0f && yhi <= Hf - 1.0f;
    return SampleWin{X0, Y0, max(0, X1 - X0 + 1), max(0, Y1 - Y0 + 1), fastdiv ? 1 : 0, sparse, interior ? 1 : 0};
}


// One pose of stage COST on the workgroup's LDS tile.
// The window is processed in chunks of at most `cap` samples (the LDS tile): one chunk -- the window -- for every
// pose the tile holds; otherwise row bands of whole window rows (blocks of columns when one row exceeds the tile),
// each rasterised over the full stream walk with triangle windows clipped to the chunk.  The costs are functions of
// the chunks' integer counts and of the explained bitmap, which accumulate across chunks, so they do not depend on
// the chunking (the overflow launch that scored such poses before round 4 took a whole-image tile instead).
template <int STRIDE, bool COLOUR>
__device__ __forceinline__ void fused_pose(const FusedArgs& a, const FusedSmem& sm, int pose, const SampleWin& pw,
                                           int cap) {
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int s = STRIDE > 0 ? STRIDE : a.stride;
    const int ws = a.ws, nsamp = a.ws * a.hs;

    for (int i = tid; i < a.bitmap_words; i += kThreads) sm.bitmap[i] = 0u;
    if (tid < 4) sm.counters[tid] = 0;
    if (a.dbg_zs)  // debug z-samples: the samples outside the window stay 0
        for (int i = tid; i < nsamp; i += kThreads) a.dbg_zs[(size_t)pose * nsamp + i] = 0;

    const bool use_seg = a.pose_label != nullptr;
    const int32_t pl = use_seg ? a.pose_label[pose] : 0;
    FProf fp;
    // counts accumulated over the chunks (wave-uniform)
    int wave_bad = 0, wave_pts = 0;
    int32_t* cid = nullptr;
    if constexpr (COLOUR) cid = a.cid + (size_t)pose * nsamp;
    // `whole`: std::true_type where sw is the pose's window itself (raster_phase, WHOLE)
    auto chunk = [&](const SampleWin& sw, auto whole) __attribute__((always_inline)) {
        const int tn = sw.nx * sw.ny;  // samples of the chunk (tile)
        for (int i = tid; i < tn; i += kThreads) sm.zbuf[i] = INT_MAX;
        if (sw.interior) raster_phase<STRIDE, false, 2, decltype(whole)::value>(a, sm, pose, sw, nullptr, fp);
        else if (sw.fastdiv) raster_phase<STRIDE, false, 1>(a, sm, pose, sw, nullptr, fp);
        else raster_phase<STRIDE, false, 0>(a, sm, pose, sw, nullptr, fp);
        fp.mark(2);
        __syncthreads();
        fp.mark(4);
        if constexpr (COLOUR) {
            // colour id pass (cost_type 1): which triangle left each sample's minimum depth (tile-local index)
            for (int i = tid; i < tn; i += kThreads) cid[i] = INT_MAX;
            __syncthreads();
            raster_phase<STRIDE, true>(a, sm, pose, sw, cid, fp);
            __syncthreads();
        }

        // ---------------- phase 2: occlusion, unprojection, 1-NN, counts ----------------
        // per-wave point queue in the (now free) triangle ring: (tile index, kx | ky << 16) pairs
        int32_t* queue = reinterpret_cast<int32_t*>(sm.ring + wave * kRecStride);  // <= 127 pairs (kRecCap >= 128)
        int qcount = 0;
        const int grid_id = use_seg ? pl : a.num_grids;
        const bool grid_ok = use_seg ? (pl >= 0 && pl < a.num_grids) : true;
        LabelGrid g;
        if (grid_ok) g = a.grids[grid_id];
        // Radius of the query's box in cells.  A neighbour p within r of q has to fall inside the box by the SAME float
        // cell coordinate that sorted it into its cell, F(x) = fl(fl(x - o) inv_c).  Per axis |p - q| <= r (1 + 2 eps)
        // (eps = 2^-24), and with the two roundings of F, each relative eps, F(p) - F(q) <= r inv_c (1 + 3 eps)
        // + 4 eps (max(|F(p)|, |F(q)|) + 1); the sum fx0 +- rc below rounds once more, 1 eps of its value.  A query with
        // a neighbour has |F| <= n + 1, so 6 eps (n + 2) = 3.6e-7 (n + 2) cells bound all of it: kBoxRound (n + 2) with
        // n the grid's longest axis does, 2.8 times over.  With the origin tens of metres from the object (a far observed
        // point stretches the segment) this term is larger than the 1e-4 r of r_eff, which alone lost neighbours at
        // r = 0.0075 with the origin 30 m away (tests/nn_cases.py, the stretched cases).
        // The box still spans <= 2 cells per axis: cells are >= 2.02 r wide, so its width is <= 2 (1.0001 r + 1e-7)
        // / (2.02 r) + 2 kBoxRound 67 = 0.99020 + 9.9e-8 / r + 1.4e-4 < 1 cell for every r >= 1.1e-5 m (n <= 65).
        // It only adds candidates to a minimum that the exact d2 <= r2 then tests.
        constexpr float kBoxRound = 1.0e-6f;
        const float r_eff = sqrtf(a.r2) * 1.0001f + 1e-7f;
        const float box_rc = grid_ok ? r_eff * g.inv_c + kBoxRound * (float)(max(g.nx, max(g.ny, g.nz)) + 2) : 0.0f;
        int my_bad = 0;

        auto process_points = [&](int count) {
            wave_sync();
            for (int base = 0; base < count; base += kWave) {
                const int j = base + lane;
                bool is_bad = false;
                if (j < count) {
                    const int k = queue[2 * j];
                    const int kxy = queue[2 * j + 1];
                    const int32_t Z = sm.zbuf[k];
                    const int kx = kxy & 0xffff, ky = kxy >> 16;
                    // compute_point_clouds.cuh:14-22 with depth_factor (cm -> m): unproject() of pcore_raster.h written
                    // out (here and in render_cloud_kernel the call gives a different instruction schedule)
                    const float zp = (float)Z / a.depth_factor;
                    const float xp = ((float)(kx * s) - a.cx) / a.fx * zp;
                    const float yp = ((float)(ky * s) - a.cy) / a.fy * zp;
                    float best = INFINITY;
                    int bidx = 0x7fffffff;
                    if (grid_ok) {
                        const float rc = box_rc;
                        const float fx0 = (xp - g.ox) * g.inv_c, fy0 = (yp - g.oy) * g.inv_c, fz0 = (zp - g.oz) * g.inv_c;
                        const float lx = fx0 - rc, hx = fx0 + rc, ly = fy0 - rc, hy = fy0 + rc, lz = fz0 - rc, hz = fz0 + rc;
                        if (hx >= 0.0f && lx < (float)g.nx && hy >= 0.0f && ly < (float)g.ny && hz >= 0.0f && lz < (float)g.nz) {
                            const int ix0 = (int)floorf(fmaxf(lx, 0.0f)), ix1 = min(g.nx - 1, (int)floorf(hx));
                            const int iy0 = (int)floorf(fmaxf(ly, 0.0f)), iy1 = min(g.ny - 1, (int)floorf(hy));
                            const int iz0 = (int)floorf(fmaxf(lz, 0.0f)), iz1 = min(g.nz - 1, (int)floorf(hz));
                            // the radius box spans <= 2 cells per axis (cell >= 2.02 r): the <= 2 cells along x of one
                            // (y, z) row are adjacent in the CSR order, so their points form ONE range -- <= 4 ranges,
                            // fetched with independent loads, then their points as one flattened sequence four at a time
                            // (clamped loads issued together); the (distance, index) minimum does not depend on the order
                            int cb[4], ce[4];
#pragma unroll
                            for (int q = 0; q < 4; q++) {
                                const int iy = iy0 + (q & 1), iz = iz0 + (q >> 1);
                                const bool ok = iy <= iy1 && iz <= iz1;
                                const int c = g.cell_base + (iz * g.ny + iy) * g.nx + ix0;
                                cb[q] = ok ? a.cell_start[c] : 0;
                                ce[q] = ok ? a.cell_start[c + 1 + (ix1 - ix0)] : 0;
                            }
                            // the <= 4 ranges as one flattened candidate sequence, four at a time: the wave loops over its
                            // lanes' largest total instead of the sum of the per-range maxima
                            const int l0 = ce[0] - cb[0], l1 = l0 + (ce[1] - cb[1]), l2 = l1 + (ce[2] - cb[2]);
                            const int ltot = l2 + (ce[3] - cb[3]);
                            for (int k0 = 0; k0 < ltot; k0 += 4) {
                                float4 o[4];
#pragma unroll
                                for (int u = 0; u < 4; u++) {
                                    const int k = min(k0 + u, ltot - 1);
                                    const int pi = k < l0 ? cb[0] + k : k < l1 ? cb[1] + (k - l0)
                                                 : k < l2 ? cb[2] + (k - l1) : cb[3] + (k - l2);
                                    o[u] = a.grid_pts[pi];
                                }
#pragma unroll
                                for (int u = 0; u < 4; u++) {
                                    const float dx = xp - o[u].x, dy = yp - o[u].y, dz = zp - o[u].z;
                                    const float d = dx * dx + dy * dy + dz * dz;
                                    const int oi = __float_as_int(o[u].w);
                                    const bool take = k0 + u < ltot && (d < best || (d == best && oi < bidx));
                                    best = take ? d : best;
                                    bidx = take ? oi : bidx;
                                }
                            }
                        }
                    }
                    // compute_costs.cuh:201-270 (cost types 0 / 2: explained marking; type 1: colour gate first)
                    if (best > a.r2) {
                        is_bad = true;
                    } else if (bidx != 0x7fffffff) {
                        bool expl = true;
                        if constexpr (COLOUR) {
                            const int id = cid[k];
                            const float4 lr = a.tri_lab[id == INT_MAX ? 0 : id];  // a valid sample has an id
                            const float4 lo = a.obs_lab[bidx];
                            const double cd = colour::colour_distance(lo.x, lo.y, lo.z, lr.x, lr.y, lr.z);
                            expl = !(cd > (double)a.colour_thr);
                        }
                        if (expl) atomicOr(&sm.bitmap[bidx >> 5], 1u << (bidx & 31));
                        else is_bad = true;
                    }
                }
                my_bad += is_bad ? 1 : 0;
            }
            wave_sync();
        };

        // tile index k -> (ix, iy) without an integer division: (k + 0.5) / nx in float is within 1e-3 of the
        // quotient (k < 2^14), so one correction step gives the exact row
        const float inv_nx = tn > 0 ? 1.0f / (float)sw.nx : 0.0f;
        for (int base = wave * kWave; base < tn; base += kThreads) {
            const int k = base + lane;
            bool valid = false;
            int kx = 0, ky = 0;
            if (k < tn && !(dbg_skip_bits(a) & 4)) {
                int iy = (int)(((float)k + 0.5f) * inv_nx), ix = k - iy * sw.nx;
                if (ix < 0) { iy--; ix += sw.nx; } else if (ix >= sw.nx) { iy++; ix -= sw.nx; }
                kx = sw.x0 + ix;
                ky = sw.y0 + iy;
                const int gk = ky * ws + kx;
                const int32_t z = sm.zbuf[k];
                // no fragment: Z = 0 whatever the source (the sampled source is read only under a fragment)
                const int32_t zf = z == INT_MAX ? 0
                                                : occlusion_rule(z, a.src_s[gk], use_seg ? (int)a.lab_s[gk] : 0, use_seg,
                                                                 pl, a.occlusion_threshold);
                if (zf != z) sm.zbuf[k] = zf;
                if (a.dbg_zs) a.dbg_zs[(size_t)pose * nsamp + gk] = zf;
                valid = zf > 0;  // depth_to_mask, compute_point_clouds.cuh:64
            }
            const uint64_t bv = __ballot(valid);
            if (valid) {
                const int q = qcount + mbcnt64(bv);
                queue[2 * q] = k;
                queue[2 * q + 1] = kx | (ky << 16);
            }
            qcount += __popcll(bv);
            wave_pts += __popcll(bv);
            if (qcount >= kWave) {
                process_points(qcount);
                qcount = 0;
            }
        }
        if (qcount > 0) process_points(qcount);
        fp.mark(5);
        for (int off = 32; off > 0; off >>= 1) my_bad += __shfl_xor(my_bad, off);
        wave_bad += __builtin_amdgcn_readfirstlane(my_bad);
    };
    if (pw.nx * pw.ny <= cap) {
        chunk(pw, std::true_type{});  // the window fits the tile (the common case: its own copy of the code, no loop state)
    } else {
        const int cw = min(pw.nx, cap), ch = max(1, cap / max(cw, 1));  // chunk columns / rows
        for (int r0 = 0; r0 < pw.ny; r0 += ch)
            for (int c0 = 0; c0 < pw.nx; c0 += cw) {
                if (r0 > 0 || c0 > 0) __syncthreads();  // the previous chunk's points are processed
                chunk(SampleWin{pw.x0 + c0, pw.y0 + r0, min(cw, pw.nx - c0), min(ch, pw.ny - r0), pw.fastdiv,
                                pw.sparse, pw.interior}, std::false_type{});
            }
    }
    // per-wave totals
    __syncthreads();  // all points counted / marked
    if (lane == 0) atomicAdd(&sm.counters[0], wave_bad);
    // number of points = number of valid samples (counted per wave above)
    int my_expl = 0;
    for (int w = tid; w < a.bitmap_words; w += kThreads) my_expl += __popc(sm.bitmap[w]);
    for (int off = 32; off > 0; off >>= 1) my_expl += __shfl_xor(my_expl, off);
    if (lane == 0) {
        atomicAdd(&sm.counters[1], my_expl);
        atomicAdd(&sm.counters[2], wave_pts);
    }
    __syncthreads();

    // ---------------- phase 3: costs (compute_costs.cuh:362-446), exact float order ----------------
    if (tid == 0) {
        const float num = (float)sm.counters[2];
        const float badf = (float)sm.counters[0];
        const float rendered_explained = num - badf;
        float rc = (num == 0.0f) ? -1.0f : badf / num;
        rc = (rc == -1.0f) ? -1.0f : rc * 100.0f;
        a.out_rc[pose] = rc;
        float ocw = 0.0f;  // the observed cost as stored
        if (a.calc_obs) {
            const float expl = (float)sm.counters[1];
            const float tot = a.pose_obs_total[pose];
            a.out_diff[pose] = rendered_explained - expl;
            float oc = tot - expl;
            oc = oc / tot;
            ocw = oc * 100.0f;
            a.out_oc[pose] = ocw;
        } else {
            if (a.out_oc) a.out_oc[pose] = 0.0f;
            if (a.out_diff) a.out_diff[pose] = 0.0f;
        }
        if (a.sel_keys) {
            const int m = a.pose_model[pose];
            const int64_t key = select_key(rc, ocw, m, a.sel_models, a.sel_base + pose);
            if (key != PCORE_KEY_NONE_DEV) atomicMin((unsigned long long*)&a.sel_keys[m], (unsigned long long)key);
        }
    }
    fp.mark(6);
    fp.flush();
}

__device__ __forceinline__ void load_pose_rows(const float* poses, int pose, float (&m)[12]) {
    const float* P = poses + (size_t)16 * pose;
#pragma unroll
    for (int i = 0; i < 12; i++) m[i] = P[i];
}

// Window launch: one workgroup per pose, LDS tile of a.tcap samples.  A pose whose window exceeds the tile is
// processed in chunks of the tile (fused_pose).
// register budget of the fused kernel: as many waves per SIMD as the most-occupied tile tier has workgroups per CU
// (6: <= 80 VGPRs; without the bound the certified fragment depth takes 82 and the kernel drops to 5 waves).  The
// colour-cost kernel (two raster passes, CIEDE2000) is left unbounded: under 80 VGPRs it spills.
#ifndef PCORE_FUSED_WAVES_PER_EU
#define PCORE_FUSED_WAVES_PER_EU PCORE_TIER_MAX
#endif
template <int STRIDE, bool COLOUR = false>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(COLOUR ? 1 : PCORE_FUSED_WAVES_PER_EU)))
fused_cost_kernel(FusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int pose = blockIdx.x;
    const WgClock wg_clock(pose);
    const FusedSmem sm = carve_smem(smem_raw, a.tcap, a.bitmap_words, COLOUR);
    // the pose window, by wave 0 only (every wave would compute the same one), shared through LDS
    if (threadIdx.x < kWave) {
        const int model = a.pose_model[pose];
        SampleWin w = {0, 0, 0, 0, 0, 0, 0};  // invalid model: nothing is rendered
        if (model >= 0 && model < a.num_models) {
            float m[12];
            load_pose_rows(a.poses, pose, m);
            w = pose_window(a, model, m, STRIDE > 0 ? STRIDE : a.stride);
        }
        if (threadIdx.x == 0) {
            sm.counters[4] = w.x0;
            sm.counters[5] = w.y0;
            sm.counters[6] = w.nx;
            sm.counters[7] = w.ny;
            sm.counters[8] = w.fastdiv;
            sm.counters[9] = w.sparse;
            sm.counters[10] = w.interior;
        }
    }
    __syncthreads();
    const SampleWin sw = {__builtin_amdgcn_readfirstlane(sm.counters[4]), __builtin_amdgcn_readfirstlane(sm.counters[5]),
                          __builtin_amdgcn_readfirstlane(sm.counters[6]), __builtin_amdgcn_readfirstlane(sm.counters[7]),
                          __builtin_amdgcn_readfirstlane(sm.counters[8]),
                          __builtin_amdgcn_readfirstlane(sm.counters[9]),
                          __builtin_amdgcn_readfirstlane(sm.counters[10])};
    const int tn = sw.nx * sw.ny;
    // Tile feedback, double-buffered by launch parity: every workgroup counts its window into this launch's
    // histogram (and, when chunked, the chunked-pose count) with atomics whose result it does not wait for;
    // workgroup 0 publishes the previous launch's counts -- complete, since launches on a stream run in order -- to
    // mapped host memory for the next call's tile choice and clears them for the launch after this one.  (A
    // last-workgroup-done publish instead made every workgroup wait on a returning atomic at exit: C2 -6 %.)
    if (threadIdx.x == 0) {
        const int par = a.fb_par;
        int b = 0;
#pragma unroll
        for (int t = 0; t < kTileTiers; t++) b += tn > a.hist_edge[t] ? 1 : 0;
        atomicAdd(&a.win_hist[par * (kTileTiers + 1) + b], 1);
        if (tn > a.tcap) atomicAdd(&a.fb_ctr[par], 1);
        if (blockIdx.x == 0 && a.fb_host) {
            const int o = (1 - par) * (kTileTiers + 1);
            for (int k = 0; k <= kTileTiers; k++) a.fb_host[k] = atomicExch(&a.win_hist[o + k], 0);
            a.fb_host[kTileTiers + 1] = atomicExch(&a.fb_ctr[1 - par], 0);
            // no system fence: the host may read a torn set, which only steers a later tile choice
            a.fb_host[kTileTiers + 2] = a.fb_seq - 1;  // the launch these counts belong to
        }
    }
    fused_pose<STRIDE, COLOUR>(a, sm, pose, sw, a.tcap);
}

// Window probe: the tier histogram of a batch's pose windows, for the tile choice of a context that has no
// published feedback yet (set_fused_tiles).  One wave per pose at a time (pose_window's corner lanes), poses strided
// over a bounded grid; waves count in registers, workgroups in LDS, and each workgroup adds its bins once (one
// address per bin: a per-pose atomic serialised, 270 us for 50 k poses).
constexpr int kProbeBlocks = 2048;
__global__ void __launch_bounds__(kThreads) window_probe_kernel(FusedArgs a, int32_t* hist) {
    constexpr int kWaves = kThreads / kWave;
    int cnt[kTileTiers + 1] = {};
    for (int pose = blockIdx.x * kWaves + (int)(threadIdx.x / kWave); pose < a.num_poses;
         pose += gridDim.x * kWaves) {  // wave-uniform
        const int model = a.pose_model[pose];
        int tn = 0;
        if (model >= 0 && model < a.num_models) {
            float m[12];
            load_pose_rows(a.poses, pose, m);
            const SampleWin w = pose_window(a, model, m, a.stride);
            tn = w.nx * w.ny;
        }
        int b = 0;
#pragma unroll
        for (int t = 0; t < kTileTiers; t++) b += tn > a.hist_edge[t] ? 1 : 0;
#pragma unroll
        for (int k = 0; k <= kTileTiers; k++) cnt[k] += b == k ? 1 : 0;
    }
    __shared__ int32_t wg_cnt[kTileTiers + 1];
    if (threadIdx.x <= kTileTiers) wg_cnt[threadIdx.x] = 0;
    __syncthreads();
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k <= kTileTiers; k++)
            if (cnt[k]) atomicAdd(&wg_cnt[k], cnt[k]);
    }
    __syncthreads();
    if (threadIdx.x <= kTileTiers && wg_cnt[threadIdx.x]) atomicAdd(&hist[threadIdx.x], wg_cnt[threadIdx.x]);
}

hipError_t launch_window_probe(const FusedArgs& a, int32_t* hist, hipStream_t s) {
    if (a.num_poses <= 0) return hipSuccess;
    const int per_wg = kThreads / kWave;
    const int blocks = std::min(kProbeBlocks, (a.num_poses + per_wg - 1) / per_wg);
    hipLaunchKernelGGL(window_probe_kernel, dim3(blocks), dim3(kThreads), 0, s, a, hist);
    return hipGetLastError();
}

// Stage CLOUD into per-pose scratch slots (the GICP source clouds): sampled raster, source occlusion,
// then the reference's compaction order (row-major samples, compute_point_clouds.cuh:290-346).
// (the fused kernel's register budget: with the fallback's vertex fetch the compiler otherwise takes 86 VGPRs, 5 waves)
template <int STRIDE>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(PCORE_FUSED_WAVES_PER_EU)))
render_cloud_kernel(FusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ int wsum[kWaves];
    __shared__ int carry_s;
    const int pose = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int s = STRIDE > 0 ? STRIDE : a.stride;
    const int ws = a.ws, nsamp = a.ws * a.hs;
    const int cap = a.tcap > 0 && a.tcap < nsamp ? a.tcap : nsamp;  // the LDS tile (samples)
    const FusedSmem sm = carve_smem(smem_raw, cap, 0);
    const int model = a.pose_model[pose];
    SampleWin sw = {0, 0, 0, 0, 0, 0, 0};
    if (model >= 0 && model < a.num_models) {
        float m[12];
        load_pose_rows(a.poses, pose, m);
        sw = pose_window(a, model, m, s);
    }
    if (tid == 0) carry_s = 0;
    const bool use_seg = a.pose_label != nullptr;
    const int32_t pl = use_seg ? a.pose_label[pose] : 0;
    FProf fp;
    float4* out = a.cloud_out + (size_t)pose * a.cloud_cap;
    // one chunk of the window (fused_pose's chunking): raster into the tile, then the chunk's valid samples appended
    // in row-major order -- row bands of whole window rows (column blocks when a row exceeds the tile) keep the
    // reference's row-major compaction order (no valid sample lies outside the window)
    auto chunk = [&](const SampleWin& cw, auto whole) __attribute__((always_inline)) {
        const int tn = cw.nx * cw.ny;
        for (int i = tid; i < tn; i += kThreads) sm.zbuf[i] = INT_MAX;
        if (cw.interior) raster_phase<STRIDE, false, 2, decltype(whole)::value>(a, sm, pose, cw, nullptr, fp);
        else if (cw.fastdiv) raster_phase<STRIDE, false, 1>(a, sm, pose, cw, nullptr, fp);
        else raster_phase<STRIDE, false, 0>(a, sm, pose, cw, nullptr, fp);
        __syncthreads();
        const float inv_nx = tn > 0 ? 1.0f / (float)cw.nx : 0.0f;
        for (int base = 0; base < tn; base += kThreads) {
            const int k = base + tid;
            int32_t zf = 0;
            int kx = 0, ky = 0;
            if (k < tn) {
                int iy = (int)(((float)k + 0.5f) * inv_nx), ix = k - iy * cw.nx;
                if (ix < 0) { iy--; ix += cw.nx; } else if (ix >= cw.nx) { iy++; ix -= cw.nx; }
                kx = cw.x0 + ix;
                ky = cw.y0 + iy;
                const int gk = ky * ws + kx;
                zf = occlusion_rule(sm.zbuf[k], a.src_s[gk], use_seg ? (int)a.lab_s[gk] : 0, use_seg, pl,
                                    a.occlusion_threshold);
            }
            const bool valid = zf > 0;
            const uint64_t b = __ballot(valid);
            if (lane == 0) wsum[wave] = __popcll(b);
            __syncthreads();
            int woff = 0, tot = 0;
            for (int w = 0; w < kWaves; w++) {
                if (w < wave) woff += wsum[w];
                tot += wsum[w];
            }
            const int carry = carry_s;
            if (valid) {
                const int o = carry + woff + mbcnt64(b);
                const float zp = (float)zf / a.depth_factor;
                const float xp = ((float)(kx * s) - a.cx) / a.fx * zp;
                const float yp = ((float)(ky * s) - a.cy) / a.fy * zp;
                if (o < a.cloud_cap) out[o] = make_float4(xp, yp, zp, 0.0f);
            }
            __syncthreads();
            if (tid == 0) carry_s = carry + tot;
            __syncthreads();
        }
    };
    if (sw.nx * sw.ny <= cap) {
        chunk(sw, std::true_type{});
    } else {
        const int cw = min(sw.nx, cap), ch = max(1, cap / max(cw, 1));
        for (int r0 = 0; r0 < sw.ny; r0 += ch)
            for (int c0 = 0; c0 < sw.nx; c0 += cw)
                chunk(SampleWin{sw.x0 + c0, sw.y0 + r0, min(cw, sw.nx - c0), min(ch, sw.ny - r0), sw.fastdiv,
                                sw.sparse, sw.interior}, std::false_type{});
    }
    if (tid == 0) a.cloud_count[pose] = carry_s < a.cloud_cap ? carry_s : a.cloud_cap;
}

hipError_t launch_render_cloud(const FusedArgs& a, hipStream_t s) {
    const int nsamp = a.ws * a.hs;
    const size_t lds = fused_lds_bytes(a.tcap > 0 && a.tcap < nsamp ? a.tcap : nsamp, 0);
    if (a.num_poses <= 0) return hipSuccess;
    if (a.stride == 8)
        hipLaunchKernelGGL(render_cloud_kernel<8>, dim3(a.num_poses), dim3(kThreads), lds, s, a);
    else
        hipLaunchKernelGGL(render_cloud_kernel<0>, dim3(a.num_poses), dim3(kThreads), lds, s, a);
    return hipGetLastError();
}

// The LDS granule (kLdsGranule, pcore_internal.h) comes from the context's DeviceInfo.
int fused_tier_samples(int t, int ws, int hs, int bitmap_words, bool colour, const DeviceInfo& d) {
    const int nsamp = ws * hs;
    const size_t granule = d.lds_granule;
    const size_t per_wg = (d.lds_per_cu / tier_wgs(t)) / granule * granule;
    const size_t fixed = fused_lds_bytes(0, bitmap_words, colour);
    if (per_wg <= fixed + 64) return 0;
    const int cap = (int)((per_wg - fixed) / 4) & ~3;
    return cap >= nsamp ? nsamp : cap;
}

hipError_t launch_fused_cost(const FusedArgs& a0, hipStream_t s) {
    if (a0.num_poses <= 0) return hipSuccess;
    const bool colour = a0.cid != nullptr;
    const int nsamp = a0.ws * a0.hs;
    FusedArgs a = a0;
    if (a.tcap <= 0 || a.tcap > nsamp) a.tcap = nsamp;
    const size_t lds = fused_lds_bytes(a.tcap, a.bitmap_words, colour);
    if (colour)
        hipLaunchKernelGGL((fused_cost_kernel<0, true>), dim3(a.num_poses), dim3(kThreads), lds, s, a);
    else if (a.stride == 8)
        hipLaunchKernelGGL(fused_cost_kernel<8>, dim3(a.num_poses), dim3(kThreads), lds, s, a);
    else
        hipLaunchKernelGGL(fused_cost_kernel<0>, dim3(a.num_poses), dim3(kThreads), lds, s, a);
    return hipGetLastError();
}

// Test hook of the colour gate's distance (pcore_debug_colour_distance): colour::colour_distance of n pairs of six
// floats (l1 a1 b1 l2 a2 b2), one thread each, called as process_points calls it on (observed, rendered).
__global__ void __launch_bounds__(256) colour_distance_test_kernel(const float* lab_pairs, double* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = lab_pairs + (size_t)6 * i;
    const float4 lo = make_float4(p[0], p[1], p[2], 0.0f), lr = make_float4(p[3], p[4], p[5], 0.0f);
    const double cd = colour::colour_distance(lo.x, lo.y, lo.z, lr.x, lr.y, lr.z);
    out[i] = cd;
}

hipError_t launch_colour_distance_test(const float* lab_pairs, double* out, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(colour_distance_test_kernel, dim3((n + 255) / 256), dim3(256), 0, s, lab_pairs, out, n);
    return hipGetLastError();
}

}  // namespace pcore
