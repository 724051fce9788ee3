// rtmi.hip -- kernels + C-ABI (include/rtmi.h) of the MI355X sampling path.  gfx950 only.
//
// Data flow of one render (all buffers in HBM):
//   scene SoA (static spheres {cx,cy,cz,r} | moving spheres | material / texture tables)
//     -> trace kernel: persistent 256-thread workgroups; the sphere SoA is staged into LDS as
//        {cx,cy,cz,r*r}; every lane owns one path (sample) at a time and runs one `color` iteration
//        (core.clj:17-41) per loop trip; lanes whose path ended are refilled from the workgroup's work
//        list (wave ballot + popcount prefix sum -> one LDS atomic per wave), so the sphere scan always
//        runs with full waves; a finished sample stores its colour at samples[tile][s][pixel]
//     -> reduce kernel: per pixel, sum over s IN SAMPLE ORDER (core.clj:52 reduce mat/add), * 1/ns
//     -> assemble kernel: tile-major -> dense frame, sqrt, *255.99, min, trunc (core.clj:54-56)
#include <hip/hip_runtime.h>
#include <rccl/rccl.h> // types and prototypes only: librccl is opened at the first multi-device gather (dlopen), never linked
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <thread>
#include <cmath>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "rtmi.h"
#include "rtmi_device.h"

using namespace rtmi;

#define RTMI_EXPORT extern "C" __attribute__((visibility("default")))

// =====================================================================================================
// kernels
// =====================================================================================================
namespace {

constexpr int kBlock = RTMI_TRACE_BLOCK;      // (the probe kernels traverse the tree too: same workgroup size as the trace kernel, see RTMI_BVH_STRIDE)
constexpr int kTraceBlock = RTMI_TRACE_BLOCK; // threads per workgroup of the trace kernel
// Diagnostic build only (make stamps -> librtmi_stamps.so): per-phase wave ticks and lane-ticks (ph_stamp, rtmi_device.h), summed over the
// launch's waves into g_phase and printed to stderr after every render, with the workgroups' start / end times.  Never defined in the
// shipped library.
#ifdef RTMI_STAMPS
__device__ unsigned long long g_wg_t[2][4096]; // s_memrealtime (100 MHz) at workgroup start / end
__device__ inline unsigned long long real_now() { unsigned long long t; asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory"); return t; }
#define RTMI_STAMP_DECL const unsigned long long st_wg0 = real_now(); \
    if (lane == 0) for (int k_ = 0; k_ < 3 * PH_SLOTS + 2; ++k_) g_ph[threadIdx.x >> 6][k_] = 0; \
    ph_stamp(-1); for (int k_ = 0; k_ < 32; ++k_) ph_stamp(PH_CAL);
#define RTMI_STAMP_FLUSH(cnt) if (lane == 0) for (int k_ = 0; k_ < 3 * PH_SLOTS; ++k_) if (g_ph[threadIdx.x >> 6][k_]) atomicAdd(&g_phase[k_], g_ph[threadIdx.x >> 6][k_]); \
    __syncthreads(); if (threadIdx.x == 0 && blockIdx.x < 4096) { g_wg_t[0][blockIdx.x] = st_wg0; g_wg_t[1][blockIdx.x] = real_now(); }
#else
#define RTMI_STAMP_DECL
#define RTMI_STAMP_FLUSH(cnt)
#endif
#ifndef RTMI_MIN_WAVES
#define RTMI_MIN_WAVES 4
#endif
#ifndef RTMI_EXT_MIN_WAVES
#define RTMI_EXT_MIN_WAVES RTMI_MIN_WAVES // waves per SIMD the mixed-kind (EXT) instantiations are compiled for
#endif

struct TraceParams {
    int nx, ny, depth;
    u64 seed;
    int tiles_x;
    int n_local_tiles;
    const int *tile_ids;   // [n_local_tiles] global tile index (row-major over tiles)
    int s_begin, s_count;  // samples [s_begin, s_begin + s_count) of every pixel in this pass
    void *samples;         // [n_local_tiles * s_count][64][3] real; [..][64][4] when the launch defers (defer_mat >= 0)
    u64 *counters;         // [0] += ray segments (metrics total-rays, core.clj:24)
    int prims_per_tile;    // static spheres per LDS tile
    int n_ptiles;          // number of LDS tiles the static spheres are cut into
    unsigned *queue;       // work queue head of this pass (zeroed before the launch): next unclaimed work item
    unsigned total_items;  // n_local_tiles * s_count * 64
    unsigned qblock;       // work items a wave claims per queue access (a multiple of 64)
    int suspend_lanes;     // time-sliced traversal: hand the wave back when fewer lanes than this are still in the tree (0: never)
    int rx0, ry0, rx1, ry1; // output region (row 0 = top): pixels outside it are not traced (whole frame: 0, 0, nx, ny)
    u64 *trav;             // COUNT instantiations: [0] += AABB slab tests (metrics aabb.intersection.total, hitable.clj:39), [1] += exact primitive tests
    int susp_off;          // mixed-kind (EXT) BVH kernels: word offset of the parked cursors in LDS = stack levels of THIS scene's tree x RTMI_BVH_STRIDE
    int stash_off;         // mixed-kind kernels: word offset of the camera-ray stash in LDS (behind the stack and the parked cursors; 0 for the scan)
    double rnx, rny;       // RN(1 / nx), RN(1 / ny): the FP64 kernels divide the jittered pixel coordinates through div_const
    int fixed_rays;        // thin lens whose offset (+-0, +-0, +-0) changes no bit of a ray's origin or direction (camera_fixed_rays): the lens disk loop only counts its draws
    int defer_mat;         // the launch defers (the kernel is a DEFER twin): paths ending on this material (DevScene::defer_mat) are stored as {atten, ny} and finished by
                           // the fold; -1: every sample is finished here and stored as 3 reals
};
#ifndef RTMI_QUEUE_BLOCK
#define RTMI_QUEUE_BLOCK 256
#endif
#ifndef RTMI_EXT_NO_STASH
#define RTMI_EXT_NO_STASH 0 // 1: the EXT (f3 / f4) instantiations refill per trip (17 VGPRs fewer)
#endif
#ifndef RTMI_EXT_LDS_STASH
#define RTMI_EXT_LDS_STASH 1 // the mixed-kind instantiations keep the camera-ray stash in LDS (11 or 17 words per entry), not in 17 VGPRs: they stand at the 128-VGPR limit of 4 waves per SIMD
#endif
#ifndef RTMI_STASH
#define RTMI_STASH 1 // camera rays generated 64 at a time at full wave width into a register stash (0: per trip, for the dead lanes only)
#endif
constexpr unsigned kQueueBlock = RTMI_QUEUE_BLOCK; // work items a wave claims per queue access at least: 4 chunks = one tile x 4 consecutive samples

// The sample record of a launch that defers: 4 reals per work item, 16-byte stores and loads (two in FP64, one in FP32); a (tile, sample) row is 64 records, contiguous
__device__ inline void store_record4(void *samples, unsigned item, const double *rgb, double w) {
    double2 *o = reinterpret_cast<double2 *>(samples) + (size_t)item * 2;
    o[0] = make_double2(rgb[0], rgb[1]); o[1] = make_double2(rgb[2], w);
}
__device__ inline void store_record4(void *samples, unsigned item, const float *rgb, float w) {
    reinterpret_cast<float4 *>(samples)[item] = make_float4(rgb[0], rgb[1], rgb[2], w);
}
__device__ inline void load_record4(const double *rec, double *rgb, double &w) {
    const double2 a = reinterpret_cast<const double2 *>(rec)[0], b = reinterpret_cast<const double2 *>(rec)[1];
    rgb[0] = a.x; rgb[1] = a.y; rgb[2] = b.x; w = b.y;
}
__device__ inline void load_record4(const float *rec, float *rgb, float &w) {
    const float4 a = *reinterpret_cast<const float4 *>(rec);
    rgb[0] = a.x; rgb[1] = a.y; rgb[2] = a.z; w = a.w;
}
// The folds of a deferring render (reduce_kernel, frame_fold_kernel: DEFER): lane l of a tile's wave owns PIXEL l, all three channels -- its record of sample s is
// 64 (entry s_count + s) + l, a contiguous 2 KB (1 KB) per wave --, where the 3-real folds own elements l, l + 64, l + 128.  Only the thread-to-element mapping
// differs: element e of a tile lies where it lay, and per element the additions run s = 0, 1, 2, ... as before.
// One sample of the lane's pixel: the record, finished (finish_deferred) if the trace kernel left it to the fold.  A row without a deferred record -- a tile
// that sees no sky -- skips that code with one wave-uniform branch.  `use`: the pixel lies inside the region (the records of the others were never written).
template <typename R> __device__ inline void fold_record4(const R *rec, const GradientU<R> &q, bool use, R *v) {
    R w;
    load_record4(rec, v, w);
    const bool deferred = use && !SampleTag<R>::is(w);
    if (__any(deferred ? 1 : 0)) {
        if (deferred) finish_deferred<R>(q, w, v[0], v[1], v[2]);
    }
}
// element k of the lane (k = 0, 1, 2) within its tile's 192, and the pixel it belongs to
template <bool DEFER> __device__ inline int fold_elem(int l, int k) { return DEFER ? 3 * l + k : l + 64 * k; }
template <bool DEFER> __device__ inline int fold_pixel(int l, int k) { return DEFER ? l : (l + 64 * k) / 3; }

template <typename R> __device__ inline const R *stat4_of(SceneRef sc);
// Stage static spheres [first, first+count) into LDS as {cx, cy, cz, r*r} (hitable.clj:188: (* radius radius)).
template <typename R> __device__ inline void stage_prims(SceneRef sc, Prim4<R> *lds, int first, int count) {
    for (int i = threadIdx.x; i < count; i += blockDim.x) {
        const R *g = stat4_of<R>(sc) + (size_t)(first + i) * 4;
        Prim4<R> p;
        p.cx = g[0]; p.cy = g[1]; p.cz = g[2]; p.r2 = g[3];
        lds[i] = p;
    }
}

template <typename R> __device__ inline const R *stat4_of(SceneRef sc);
template <> __device__ inline const double *stat4_of<double>(SceneRef sc) { return sc.stat4_d; }
template <> __device__ inline const float *stat4_of<float>(SceneRef sc) { return sc.stat4_f; }

// the FP32 cull exists for the FP64 path only; RTMI_F32 falls back to the plain scalar-cache scan
// ANY (the any-hit queries): the scans may stop once every lane holds a hit, and a lane that holds one skips the moving spheres
template <bool ANY = false>
__device__ inline void scan_cull_dispatch(SceneRef sc, const Path<double> &P, double a, double tmin, double &best_t, int &best_i) {
    scan_all_cull<ANY>(sc, P, a, tmin, best_t, best_i);
}
template <bool ANY = false>
__device__ inline void scan_cull_dispatch(SceneRef sc, const Path<float> &P, float a, float tmin, float &best_t, int &best_i) {
    scan_static_pipe<float, false, ANY>(ScalarPrims<float>(sc.stat4_f), sc.n_static, 0, P, a, tmin, best_t, best_i);
    if (best_i >= 0) best_i = sc.stat_orig[best_i];
    if (ANY && best_i >= 0) return;
    if (sc.n_moving > 0) {
        int best_orig = best_i >= 0 ? best_i : 0x7fffffff, scan_i = -1;
        scan_moving<float>(sc, P, a, tmin, best_t, scan_i, best_orig);
        if (scan_i >= 0) best_i = best_orig;
    }
}


// hit? of the whole world for the lane's ray (closest hit, t in (t-min, t-max); core.clj:25 passes 0.001, Float/MAX_VALUE).
// MULTI (LDS variants only): the static spheres do not fit one LDS tile; every thread of the workgroup must call this.
// section 8(f3) scenes (FP64 only): BVH or culled flat scan over mixed primitive kinds with the any-order tie rule
// MSEQ: the instantiations for RTMI_MEDIA_HITLIST (1) and RTMI_MEDIA_NARROWED (2) worlds (their own kernels: the plain mixed-kind kernels keep their registers)
// ANY (the any-hit queries, MSEQ = 0 only -- the media_seq worlds run the closest-hit search as it is): only best_i >= 0 is wanted.  The media come first
// and see the caller's interval whatever the surfaces do; a lane one of them hits is done, the others scan the surfaces against the initial t-max
// and leave at the first accepted primitive (scan_bvh_ext).
template <bool SLICED = false, bool COUNT = false, int MSEQ = 0, bool ANY = false>
__device__ inline void intersect_ext(SceneRef sc, int *stack, bool bvh, Path<double> &P, bool active, double tmin, double tmax, double &best_t, int &best_i,
                                     bool *mid = nullptr, int min_lanes = 0, unsigned *cnt = nullptr, int susp_off = RTMI_BVH_STACK * RTMI_BVH_STRIDE) {
    best_t = tmax; best_i = -1;
    if (!active) return;
    const double a = dot3(P.dx, P.dy, P.dz, P.dx, P.dy, P.dz);
    ExtHit H = {tmax, 0x7fffffff, -1};
    if (MSEQ == 2) { // (an instantiation of its own: with both list forms inlined side by side one of the kernels went to 248 registers and scratch)
        // RTMI_MEDIA_NARROWED: Hitlists holding media BELOW bvh-nodes (round 4).  A bvh-node hands its children the un-narrowed interval (hitable.clj:99-105), a Hitlist
        // hands every item the closest hit of the items before it (hitable.clj:15-26): call k of the media sequence sees the closest hit among the primitives
        // [media_lo[k], media_idx[k]) -- the items before it in its own (possibly nested) Hitlist -- or the caller's t-max when that range is empty.  The items of one
        // Hitlist are contiguous in the flattened order, so the narrowing state is a running closest hit over that list: its surfaces are scanned piece by piece
        // between its media (index-restricted scan: such lists are short), every medium's candidate joins it.  The world's closest hit is then the fold of ALL
        // surfaces (one traversal, below) and of the media's candidates -- in any order (ExtHit).
        MediumChord chord = medium_chord_begin(P);
        ExtHit Hrun = {tmax, 0x7fffffff, -1};
        int cur_lo = -1, scanned_to = 0;
        for (int k = 0; k < sc.n_media; ++k) {
            const int m = sc.media_idx[k], lo = sc.media_lo[k];
            if (lo >= m) { ext_medium_test(sc, m, P, tmin, tmax, H, chord, COUNT ? cnt : nullptr); continue; } // un-narrowed: a medium reached through bvh-nodes only
            if (lo != cur_lo) { Hrun.t = tmax; Hrun.F = 0x7fffffff; Hrun.W = -1; cur_lo = lo; scanned_to = lo; }
            if (m > scanned_to) scan_all_cull_ext(sc, P, a, tmin, Hrun, scanned_to, m);
            double tm = 0.0;
            if (ext_medium_test(sc, m, P, tmin, Hrun.any() ? Hrun.t : tmax, Hrun, chord, COUNT ? cnt : nullptr, &tm)) ext_update(H, tm, m, true);
            scanned_to = m + 1;
        }
        if (bvh) scan_bvh_ext<false, COUNT>(sc, stack, P, a, tmin, H, nullptr, false, 0, cnt);
        else if (sc.small_scan) scan_small_ext(sc, P, tmin, H);
        else scan_all_cull_ext(sc, P, a, tmin, H);
        best_i = ext_winner(H);
        if (best_i >= 0) best_t = H.t;
        return;
    }
    if (MSEQ == 1) {
        // RTMI_MEDIA_HITLIST: the world is a Hitlist (hitable.clj:15-26: (hit? item r t-min closest-so-far), item after item).  Surfaces may be
        // folded in any order (ExtHit reproduces the list's tie rule), so the list is scanned in pieces: the surfaces before the first medium,
        // that medium with the t-max the list would hand it -- the closest hit so far --, the surfaces up to the next medium, and so on.  (These
        // scenes run the instantiation without time-slicing: media_seq and SLICED never meet.)
        int prev = 0;
        MediumChord chord = medium_chord_begin(P);
        for (int k = 0; k <= sc.n_media; ++k) {
            const int m = k < sc.n_media ? sc.media_idx[k] : sc.n_all;
            if (m > prev) {
                if (bvh) scan_bvh_ext<false, COUNT>(sc, stack, P, a, tmin, H, nullptr, false, 0, cnt, prev, m);
                else if (sc.small_scan) scan_small_ext(sc, P, tmin, H, prev, m);
                else scan_all_cull_ext(sc, P, a, tmin, H, prev, m);
            }
            if (k < sc.n_media) ext_medium_test(sc, m, P, tmin, H.any() ? H.t : tmax, H, chord, COUNT ? cnt : nullptr);
            prev = m + 1;
        }
        best_i = ext_winner(H);
        if (best_i >= 0) best_t = H.t;
        return;
    }
    // Media FIRST (RTMI_MEDIA_DESCENT: every medium's hit? sees the caller's un-narrowed interval, hitable.clj:99-105, so its result -- and its draws, the only
    // draws of a hit? -- do not depend on the surfaces; ExtHit folds candidates in any order).  The surfaces' traversal then starts with the closest MEDIUM hit as
    // its bound: a path scattering inside make-final's subsurface sphere (mean free path 5; a third of that scene's segments) or ending in its haze no longer
    // walks the tree with an unbounded interval before its medium is asked.  The reference's call order is kept: primitive-index order = the order its descent
    // calls the media (and draws).  A resumed lane (time-sliced traversal) evaluated its media when its segment began; they ride in its parked hit state.
    if (!(SLICED && bvh && *mid)) {
        MediumChord chord = medium_chord_begin(P);
        for (int k = 0; k < sc.n_media; ++k) ext_medium_test(sc, sc.media_idx[k], P, tmin, tmax, H, chord, COUNT ? cnt : nullptr, nullptr, k);
        RTMI_PH(PH_MEDIA)
    }
    if (ANY && H.any()) { best_i = ext_winner(H); best_t = H.t; return; }
    if (bvh) {
        if (SLICED) {
            const bool done = scan_bvh_ext<true, COUNT>(sc, stack, P, a, tmin, H, stack + susp_off, *mid, min_lanes, cnt);
            *mid = !done;
            if (!done) return;
        } else scan_bvh_ext<false, COUNT, ANY>(sc, stack, P, a, tmin, H, nullptr, false, 0, cnt);
    } else if (sc.small_scan) scan_small_ext<ANY>(sc, P, tmin, H); // (wave-uniform)
    else scan_all_cull_ext<ANY>(sc, P, a, tmin, H);
    RTMI_PH(PH_BVH_POST)
    best_i = ext_winner(H);
    if (best_i >= 0) best_t = H.t;
}
template <bool SLICED = false, bool COUNT = false, int MSEQ = 0, bool ANY = false>
__device__ inline void intersect_ext(SceneRef, int *, bool, Path<float> &, bool, float, float tmax, float &best_t, int &best_i, bool * = nullptr, int = 0, unsigned * = nullptr, int = 0) { best_t = tmax; best_i = -1; }

// NOGRID: the plain (not time-sliced) RENDER kernel -- never launched on a scene with an entry grid, so it carries no code for one (the probe
// kernels, also not time-sliced, do: they walk a long segment's pieces in a loop of their own)
// ANY (query_kernel's any-hit instantiations; never SLICED, never the LDS-staged scans): best_i >= 0 iff the closest-hit search would find a hit; which
// primitive and which t is arbitrary
template <typename R, bool MULTI, int VARIANT, bool EXT = false, bool COUNT = false, bool SLICED = false, int MSEQ = 0, bool NOGRID = false, bool ANY = false>
__device__ inline void intersect_world(SceneRef sc, Prim4<R> *lds, int prims_per_tile, int n_ptiles, Path<R> &P,
                                       bool active, R tmin, R tmax, R &best_t, int &best_i, unsigned *cnt = nullptr, bool *mid = nullptr, int min_lanes = 0,
                                       int susp_off = RTMI_BVH_STACK * RTMI_BVH_STRIDE) {
    if (EXT) { intersect_ext<SLICED, COUNT, MSEQ, ANY && MSEQ == 0>(sc, reinterpret_cast<int *>(lds), VARIANT == SCAN_BVH, P, active, tmin, tmax, best_t, best_i, mid, min_lanes, cnt, susp_off); return; }
    best_t = tmax;
    best_i = -1;
    const R a = dot3(P.dx, P.dy, P.dz, P.dx, P.dy, P.dz);
    if (VARIANT == SCAN_BVH) { // RTMI_ACCEL_BVH; `lds` is the traversal stack, followed by the suspended lanes' state when the traversal is time-sliced
        int *stack = reinterpret_cast<int *>(lds);
        if (active) {
            if (SLICED) {
                const bool done = scan_bvh<R, COUNT, true>(sc, stack, P, a, tmin, best_t, best_i, [&]() { scan_cull_dispatch(sc, P, a, tmin, best_t, best_i); }, cnt,
                                                           stack + susp_off, *mid, min_lanes);
                *mid = !done;
            } else scan_bvh<R, COUNT, false, !NOGRID, ANY>(sc, stack, P, a, tmin, best_t, best_i, [&]() { scan_cull_dispatch<ANY>(sc, P, a, tmin, best_t, best_i); }, cnt);
        }
        return;
    }
    if (VARIANT == SCAN_SGPR_CULL) { // all primitives, original order; returns the original index
        if (active) scan_cull_dispatch<ANY>(sc, P, a, tmin, best_t, best_i);
        return;
    }
    if (VARIANT == SCAN_SGPR) {
        if (active) scan_static_pipe<R, false, ANY>(ScalarPrims<R>(stat4_of<R>(sc)), sc.n_static, 0, P, a, tmin, best_t, best_i);
    } else if (!MULTI) {
        if (active) {
            if (VARIANT == SCAN_LDS_PIPE) scan_static_pipe<R, true>(LdsPrims<R>{lds}, sc.n_static, 0, P, a, tmin, best_t, best_i);
            else scan_static<R>(lds, sc.n_static, 0, P, a, tmin, best_t, best_i);
        }
    } else {
        for (int tile = 0; tile < n_ptiles; ++tile) {
            const int first = tile * prims_per_tile;
            const int count = min(prims_per_tile, sc.n_static - first);
            __syncthreads();
            stage_prims<R>(sc, lds, first, count);
            __syncthreads();
            if (active) {
                if (VARIANT == SCAN_LDS_PIPE) scan_static_pipe<R, true>(LdsPrims<R>{lds}, count, first, P, a, tmin, best_t, best_i);
                else scan_static<R>(lds, count, first, P, a, tmin, best_t, best_i);
            }
        }
    }
    // static spheres were scanned in their own (original relative) order; convert to the original index, then the
    // moving spheres, with ties resolved by original index (first in Hitlist order wins, hitable.clj:20)
    if (active) {
        if (best_i >= 0) best_i = sc.stat_orig[best_i];
        if (sc.n_moving > 0 && !(ANY && best_i >= 0)) {
            int best_orig = best_i >= 0 ? best_i : 0x7fffffff, scan_i = -1;
            scan_moving<R>(sc, P, a, tmin, best_t, scan_i, best_orig);
            if (scan_i >= 0) best_i = best_orig;
        }
    }
}

// core.clj:43-51: jittered (u, v) for sample s of pixel (i, j), then the camera ray.
template <typename R> __device__ inline void start_sample(SceneRef sc, const TraceParams &tp, int i, int j, int s, Path<R> &P) {
    seed_stream(P, sample_key(tp.seed, (u64)j * (u64)tp.nx + (u64)i, (u64)s), 0u);
    const R u = ((R)(float)i + next_uniform(P)) / (R)tp.nx;
    const R v = ((R)(float)j + next_uniform(P)) / (R)tp.ny;
    RTMI_PH(PH_GEN_KEY)
    get_ray<R>(sc, u, v, P);
    P.ar = P.ag = P.ab = R(1);
    P.depth = tp.depth;
}

// (i + u) / nx of start_sample: nx is a launch constant, so the FP64 kernels take the correctly rounded quotient from div_const (rn = RN(1 / n), one host
// division per launch; 0 <= x <= n < 2^31, so no operand is scaled and Markstein's correction applies); the FP32 kernels keep their division
__device__ inline double pixel_quot(double x, int n, double rn) { return div_const(x, (double)n, rn); }
__device__ inline float pixel_quot(float x, int n, double) { return x / (float)n; }

#ifndef RTMI_GEN_PLAIN
#define RTMI_GEN_PLAIN 0 // 1: the stash refills generate with start_sample under the item mask, as before the wave-wide routine (A/B and the stamps' "before")
#endif
// What a wave keeps between the generations of one tile: a claim is qblock / 64 consecutive chunks = the same 64 pixels, samples s, s + 1, ...,
// so the tile's origin (wave-uniform) and each lane's inner pixel hash mix64(seed ^ GOLD (pix + 1)) are computed when the tile changes only.
// KEEP = false (the instantiations that stand at their register limit): nothing is carried, every generation recomputes them.
struct GenTile { int tile, x0, y0; u64 hpix; };
// One generation: chunk (wave-uniform) = 64 consecutive work items = sample s of the 64 pixels of one tile, lane l its pixel l.  The WHOLE wave calls
// (wave-uniform control flow); returns whether the lane's item lies inside the image and region -- the others come along as helpers of the
// cooperative disk sampler and their Q is never read.  Per lane the same stream and the same operations as start_sample.
template <typename R, bool KEEP> __device__ inline bool generate_camera_rays(SceneRef sc, const TraceParams &tp, unsigned chunk, int lane, GenTile &g, Path<R> &Q) {
    const int tile_local = (int)(chunk / (unsigned)tp.s_count);
    const int s = tp.s_begin + (int)(chunk - (unsigned)tile_local * (unsigned)tp.s_count);
#if RTMI_GEN_PLAIN
    const int gtile = tp.tile_ids[tile_local];
    const int x = (gtile % tp.tiles_x) * RTMI_TILE + (lane & 7), y = (gtile / tp.tiles_x) * RTMI_TILE + (lane >> 3);
    const bool has = x >= tp.rx0 && x < tp.rx1 && y >= tp.ry0 && y < tp.ry1;
    if (has) start_sample<R>(sc, tp, x, tp.ny - 1 - y, s, Q);
    return has;
#else
    if (!KEEP || tile_local != g.tile) { // wave-uniform
        const int gtile = tp.tile_ids[tile_local];
        g.x0 = (gtile % tp.tiles_x) * RTMI_TILE; g.y0 = (gtile / tp.tiles_x) * RTMI_TILE;
        const int i = g.x0 + (lane & 7), j = tp.ny - 1 - (g.y0 + (lane >> 3));
        g.hpix = mix64(tp.seed ^ (RTMI_GOLD * ((u64)j * (u64)tp.nx + (u64)i + 1)));
        g.tile = tile_local;
    }
    const int x = g.x0 + (lane & 7), y = g.y0 + (lane >> 3), j = tp.ny - 1 - y; // j = ny-1-y (core.clj:105)
    const bool has = x >= tp.rx0 && x < tp.rx1 && y >= tp.ry0 && y < tp.ry1;
    seed_stream(Q, mix64(g.hpix + 0xD1B54A32D192ED03ULL * ((u64)s + 1)), 0u); // = sample_key(seed, j nx + x, s)
    const R ju = next_uniform(Q), jv = next_uniform(Q);
    const R u = pixel_quot((R)(float)x + ju, tp.nx, tp.rnx);
    const R v = pixel_quot((R)(float)j + jv, tp.ny, tp.rny);
    RTMI_PH(PH_GEN_KEY)
    get_ray_wave<R>(sc, tp.fixed_rays != 0, has, u, v, Q);
    return has;
#endif
}

// SLICE: time-sliced BVH traversal (section 5.1b of DESIGN.md); the plain instantiation is kept for scenes whose tree is too small to gain
// LST: the sphere (non-EXT) time-sliced BVH kernel with the camera-ray stash in LDS and stack columns sized by the scene's tree (launch site: when it fits)
// DEFER: the twin a launch that defers runs (TraceParams::defer_mat >= 0; the tree kernels of sphere-only scenes have one): paths that end on the scene's deferred
// emitter are stored unfinished, 4 reals per record.  Every other instantiation is compiled without a trace of it
template <typename R, bool MULTI, int VARIANT, bool EXT = false, bool COUNT = false, bool SLICE = true, int MSEQ = 0, bool LST = false, bool DEFER = false>
// (the Hitlist-with-media (MSEQ) and the counting (COUNT) instantiations of the mixed-kind kernels need more than the 128 VGPRs of four waves per SIMD: rather
// than spill, they are compiled for three -- rare worlds and a diagnostic; the kernels the benchmarks run keep four)
__global__ void __launch_bounds__(kTraceBlock, EXT ? ((MSEQ != 0 || COUNT) ? 3 : RTMI_EXT_MIN_WAVES) : RTMI_MIN_WAVES) trace_kernel(ScenePtr scp, TraceParams tp) {
    SceneRef sc = *scp;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Prim4<R> *lds = reinterpret_cast<Prim4<R> *>(smem);
    const int lane = threadIdx.x & 63;
    if (!MULTI && VARIANT < SCAN_SGPR) stage_prims<R>(sc, lds, 0, sc.n_static);
    __syncthreads();

    // Work distribution: one queue for the whole launch.  A work item is one sample of one pixel; item m belongs to chunk
    // m / 64 = (local tile m / (64 s_count), sample s_begin + (m / 64) % s_count), pixel m % 64 of that 8x8 tile.  Each WAVE
    // claims kQueueBlock consecutive items at a time with one global atomic and hands them to its dead lanes; no wave idles
    // while the queue holds work, whatever the other waves' paths do.  (Which wave renders an item never affects the result:
    // the RNG stream is a function of (seed, pixel, sample) only.)
    const unsigned total_items = tp.total_items;
    unsigned w_cur = 0, w_end = 0; // this wave's claimed range [w_cur, w_end): wave-uniform
    Path<R> P;
    P.ox = P.oy = P.oz = P.dx = P.dy = P.dz = P.time = R(0);
    P.ar = P.ag = P.ab = R(0);
    seed_stream(P, 0ull, 0u); P.depth = 0;
    bool alive = false;
    bool exhausted = (total_items == 0);
    unsigned out_item = 0; // work item of the lane's path: its colour goes to samples[out_item]
    constexpr bool LSTASH = (EXT && RTMI_STASH && RTMI_EXT_LDS_STASH && !RTMI_EXT_NO_STASH) || LST;
    constexpr bool STASH = RTMI_STASH && !(EXT && RTMI_EXT_NO_STASH) && !LSTASH;
    // LSTASH: entry e of wave w = words lst[k * kTraceBlock + e], k = 0..5 direction, 6..7 time, 8..9 stream state, 10 work item (-1: none), 11..16 origin
    // (only written / read when the camera's rays do not all start at one point).  Written and read by the same wave only.
    int *const lst = reinterpret_cast<int *>(smem) + tp.stash_off + (threadIdx.x & ~63);
    R st_ox = R(0), st_oy = R(0), st_oz = R(0), st_dx = R(0), st_dy = R(0), st_dz = R(0), st_time = R(0); // the stash: one generated camera ray per lane
    u64 st_rs = 0;
    unsigned st_item = 0xffffffffu;
    unsigned s_head = 64u; // wave-uniform: entries [s_head, 64) are unclaimed
    constexpr bool KEEP = LST; // the per-tile invariants cost two VGPRs across the path loop: kept where the kernel has them to spare (profiles/camera_rays_resources.txt)
    GenTile gen = {-1, 0, 0, 0ull};
    unsigned nrays = 0;
    unsigned ntrav[2] = {0u, 0u};
    const R tmin = R(0.001), tmax = Real<R>::tmax();
    constexpr bool SLICED = SLICE && VARIANT == SCAN_BVH && !MULTI;
    bool mid = false; // this lane's segment is suspended inside the tree (SLICED)

    RTMI_STAMP_DECL
    for (;;) {
        RTMI_PH(PH_LOOP) // loop overhead / tail
        // ---- refill dead lanes ------------------------------------------------------------------------------------------
        if (LSTASH) {
        for (;;) { // wave-uniform control flow; as the register stash below with the entries in LDS
            const u64 dead = __ballot(!alive);
            if (dead == 0) break;
            if (s_head == 64u) {
                if (exhausted) break;
                if (w_cur == w_end) {
                    unsigned base = 0;
                    if (lane == 0) base = atomicAdd(tp.queue, tp.qblock);
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (base >= total_items) { exhausted = true; break; }
                    w_cur = base;
                    w_end = min(base + tp.qblock, total_items);
                }
                const unsigned m = w_cur + (unsigned)lane; // (w_cur is a multiple of 64: lane l holds pixel l of chunk w_cur / 64)
                Path<R> Q;
                const bool has = generate_camera_rays<R, KEEP>(sc, tp, w_cur >> 6, lane, gen, Q);
                w_cur += 64u;
                unsigned item = 0xffffffffu; // (an item outside the image / region: an empty entry; work items are 32-bit UNSIGNED -- C4 has 2.1e9 per pass)
                if (has) {
                    int w0, w1;
                    best_to_words<R>(Q.dx, w0, w1); lst[lane] = w0; lst[kTraceBlock + lane] = w1;
                    best_to_words<R>(Q.dy, w0, w1); lst[2 * kTraceBlock + lane] = w0; lst[3 * kTraceBlock + lane] = w1;
                    best_to_words<R>(Q.dz, w0, w1); lst[4 * kTraceBlock + lane] = w0; lst[5 * kTraceBlock + lane] = w1;
                    best_to_words<R>(Q.time, w0, w1); lst[6 * kTraceBlock + lane] = w0; lst[7 * kTraceBlock + lane] = w1;
                    lst[8 * kTraceBlock + lane] = (int)(unsigned)Q.rs; lst[9 * kTraceBlock + lane] = (int)(unsigned)(Q.rs >> 32);
                    if (!sc.cam_fixed_origin) {
                        best_to_words<R>(Q.ox, w0, w1); lst[11 * kTraceBlock + lane] = w0; lst[12 * kTraceBlock + lane] = w1;
                        best_to_words<R>(Q.oy, w0, w1); lst[13 * kTraceBlock + lane] = w0; lst[14 * kTraceBlock + lane] = w1;
                        best_to_words<R>(Q.oz, w0, w1); lst[15 * kTraceBlock + lane] = w0; lst[16 * kTraceBlock + lane] = w1;
                    }
                    item = m;
                    RTMI_PH(PH_REFILL_GEN)
                }
                lst[10 * kTraceBlock + lane] = (int)item;
                s_head = 0u;
            }
            const unsigned avail = 64u - s_head, nd = (unsigned)__popcll(dead);
            const unsigned rank = (unsigned)__popcll(dead & ((1ull << lane) - 1ull));
            if (!alive && rank < avail) {
                const int e = (int)(s_head + rank);
                const unsigned item = (unsigned)lst[10 * kTraceBlock + e];
                if (item != 0xffffffffu) {
                    P.dx = best_from_words<R>(lst[e], lst[kTraceBlock + e]); P.dy = best_from_words<R>(lst[2 * kTraceBlock + e], lst[3 * kTraceBlock + e]);
                    P.dz = best_from_words<R>(lst[4 * kTraceBlock + e], lst[5 * kTraceBlock + e]); P.time = best_from_words<R>(lst[6 * kTraceBlock + e], lst[7 * kTraceBlock + e]);
                    P.rs = (u64)(unsigned)lst[8 * kTraceBlock + e] | ((u64)(unsigned)lst[9 * kTraceBlock + e] << 32);
                    if (sc.cam_fixed_origin) { P.ox = (R)sc.cam[0]; P.oy = (R)sc.cam[1]; P.oz = (R)sc.cam[2]; }
                    else {
                        P.ox = best_from_words<R>(lst[11 * kTraceBlock + e], lst[12 * kTraceBlock + e]); P.oy = best_from_words<R>(lst[13 * kTraceBlock + e], lst[14 * kTraceBlock + e]);
                        P.oz = best_from_words<R>(lst[15 * kTraceBlock + e], lst[16 * kTraceBlock + e]);
                    }
                    P.ar = P.ag = P.ab = R(1);
                    P.depth = tp.depth;
                    out_item = item;
                    alive = true;
                }
            }
            s_head += min(nd, avail);
        }
        } else if (STASH) {
        // Camera rays are generated 64 at a time by the WHOLE wave (key, jitter, lens disk loop, get-ray: start_sample at full
        // width) into a register stash, one entry per lane; dead lanes then pull entries across lanes (ds_bpermute): entry
        // s_head + (rank among the dead lanes).  Generating per trip for the dead lanes only ran start_sample at ~40 % width
        // every trip; now it runs at full width every ~2.5 trips.  Which lane traces an item never affects the result.
        for (;;) { // wave-uniform control flow
            const u64 dead = __ballot(!alive);
            if (dead == 0) break;
            if (s_head == 64u) {
                if (exhausted) break;
                if (w_cur == w_end) {
                    unsigned base = 0;
                    if (lane == 0) base = atomicAdd(tp.queue, tp.qblock);
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (base >= total_items) { exhausted = true; break; }
                    w_cur = base;
                    w_end = min(base + tp.qblock, total_items); // total_items and qblock are multiples of 64
                }
                const unsigned m = w_cur + (unsigned)lane; // (w_cur is a multiple of 64: lane l holds pixel l of chunk w_cur / 64)
                Path<R> Q;
                const bool has = generate_camera_rays<R, KEEP>(sc, tp, w_cur >> 6, lane, gen, Q);
                w_cur += 64u;
                st_item = 0xffffffffu; // an item outside the image / region: an empty entry
                if (has) {
                    st_ox = Q.ox; st_oy = Q.oy; st_oz = Q.oz; st_dx = Q.dx; st_dy = Q.dy; st_dz = Q.dz; st_time = Q.time; st_rs = Q.rs;
                    st_item = m;
                    RTMI_PH(PH_REFILL_GEN)
                }
                s_head = 0u;
            }
            const unsigned avail = 64u - s_head, nd = (unsigned)__popcll(dead);
            const unsigned rank = (unsigned)__popcll(dead & ((1ull << lane) - 1ull));
            const bool take = !alive && rank < avail;
            const int src = take ? (int)(s_head + rank) : lane;
            R f_ox, f_oy, f_oz;
            if (sc.cam_fixed_origin) { f_ox = (R)sc.cam[0]; f_oy = (R)sc.cam[1]; f_oz = (R)sc.cam[2]; } // wave-uniform: 6 cross-lane moves fewer per deal
            else { f_ox = __shfl(st_ox, src); f_oy = __shfl(st_oy, src); f_oz = __shfl(st_oz, src); }
            const R f_dx = __shfl(st_dx, src), f_dy = __shfl(st_dy, src), f_dz = __shfl(st_dz, src), f_time = __shfl(st_time, src);
            const u64 f_rs = __shfl(st_rs, src);
            const unsigned f_item = __shfl(st_item, src);
            if (take && f_item != 0xffffffffu) {
                P.ox = f_ox; P.oy = f_oy; P.oz = f_oz; P.dx = f_dx; P.dy = f_dy; P.dz = f_dz; P.time = f_time; P.rs = f_rs;
                P.ar = P.ag = P.ab = R(1);
                P.depth = tp.depth;
                out_item = f_item;
                alive = true;
            }
            s_head += min(nd, avail);
        }
        } else
        while (!exhausted) { // every lane of the wave takes part: the loop conditions are wave-uniform
            const u64 dead = __ballot(!alive);
            if (dead == 0) break;
            if (w_cur == w_end) {
                unsigned base = 0;
                if (lane == 0) base = atomicAdd(tp.queue, kQueueBlock);
                base = __builtin_amdgcn_readfirstlane(base);
                if (base >= total_items) { exhausted = true; break; }
                w_cur = base;
                w_end = min(base + kQueueBlock, total_items);
            }
            const unsigned avail = w_end - w_cur;
            const unsigned rank = (unsigned)__popcll(dead & ((1ull << lane) - 1ull));
            if (!alive && rank < avail) {
                const unsigned m = w_cur + rank;
                const unsigned chunk = m >> 6;
                const int l = (int)(m & 63u);
                const int tile_local = (int)(chunk / (unsigned)tp.s_count);
                const int s = tp.s_begin + (int)(chunk - (unsigned)tile_local * (unsigned)tp.s_count);
                const int gtile = tp.tile_ids[tile_local];
                const int x = (gtile % tp.tiles_x) * RTMI_TILE + (l & 7);
                const int y = (gtile / tp.tiles_x) * RTMI_TILE + (l >> 3);
                if (x >= tp.rx0 && x < tp.rx1 && y >= tp.ry0 && y < tp.ry1) {
                    start_sample<R>(sc, tp, x, tp.ny - 1 - y, s, P); // j = ny-1-y (core.clj:105)
                    out_item = m;
                    alive = true;
                }
            }
            w_cur += min((unsigned)__popcll(dead), avail);
        }
        if (MULTI) { if (!__syncthreads_or(alive ? 1 : 0)) break; }
        else { if (!__any(alive ? 1 : 0)) break; }
        RTMI_PH(PH_REFILL_DEAL) // refill: claims, dealing stash entries to dead lanes

        // ---- one iteration of `color` for every live lane ---------------------------------------------
        // SLICED (BVH kernels): the traversal hands the wave back as soon as fewer than tp.suspend_lanes lanes are still in the tree
        // (a few rays of a wave visit ten times the nodes the others do: 40 % of the node-visit trips served < 8 lanes); those lanes
        // are `mid` segment -- they sit out the shading below and resume where they stopped in the next trip, next to the new
        // segments of the others.  Once the queue is empty nothing is gained by handing back early (suspend_lanes 0).
        R best_t; int best_i;
        intersect_world<R, MULTI, VARIANT, EXT, COUNT, SLICED, MSEQ, !SLICED>(sc, lds, tp.prims_per_tile, tp.n_ptiles, P, alive, tmin, tmax, best_t, best_i, ntrav,
                                                                     &mid, exhausted ? 0 : tp.suspend_lanes, (EXT || LST) ? tp.susp_off : RTMI_BVH_STACK * RTMI_BVH_STRIDE);
        RTMI_PH(PH_BVH_POST) // intersection: what the phases inside did not book (suspend bookkeeping, call overhead)
        if (!SLICED || __any(alive && !mid)) { // a trip in which no lane finished its segment has nothing to shade
        if (alive) {
            if (!mid) ++nrays;
            R emit[3];
            if constexpr (!DEFER) { // (the call and the store exactly as they stood: these instantiations compile to the registers they had)
                const bool scat = shade_segment<R, EXT>(sc, P, best_t, best_i, nullptr, emit, mid); // a `mid` lane is a passenger: it changes nothing
                if (!mid && !scat) {
                    R *out = reinterpret_cast<R *>(tp.samples) + (size_t)out_item * 3;
                    out[0] = emit[0]; out[1] = emit[1]; out[2] = emit[2];
                    alive = false;
                    RTMI_PH(PH_STORE)
                }
            } else {
                R dny;
                bool deferred;
                const bool scat = shade_segment<R, EXT, true>(sc, P, best_t, best_i, nullptr, emit, mid, tp.defer_mat, &deferred, &dny);
                if (!mid && !scat) {
                    store_record4(tp.samples, out_item, emit, deferred ? dny : SampleTag<R>::value()); // {r, g, b, SampleTag} or {ar, ag, ab, ny}
                    alive = false;
                    RTMI_PH(PH_STORE)
                }
            }
        }
        }
        RTMI_PH(PH_STORE) // shading: what its phases did not book
    }
    RTMI_STAMP_FLUSH(tp.counters)
    // total-rays: wave reduction, one atomic per wave
    unsigned n = nrays;
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off);
    if (lane == 0 && n) atomicAdd(tp.counters, (u64)n);
    if (COUNT) {
        u64 a = ntrav[0], b = ntrav[1];
        for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off); b += __shfl_down(b, off); }
        if (lane == 0) { atomicAdd(tp.trav, a); atomicAdd(tp.trav + 1, b); }
    }
}

// core.clj:52-53: (reduce mat/add) over the samples IN ORDER, then (mul (/ 1.0 nr)) on the last pass.
// DEFER: the samples are the 4-real records of a launch that defers and a lane owns a pixel (fold_record4); grad = mat_grad[defer_mat], the scene's record in HBM.
template <typename R, bool DEFER = false>
__global__ void __launch_bounds__(kBlock) reduce_kernel(const R *__restrict__ samples, R *__restrict__ accum, double *__restrict__ tiles_linear,
                                                        const int *__restrict__ tile_ids, int tiles_x, int nx, int ny, int n_local_tiles,
                                                        int s_begin, int s_count, int ns, u64 *counters, u64 n_valid_pixels,
                                                        int rx0, int ry0, int rx1, int ry1, const double *__restrict__ grad) {
    // A (tile, sample) row is 64 pixels x 3 channels = 192 consecutive values; the sum over the samples is element-wise, so lane l of the
    // tile's wave owns elements l, l + 64, l + 128 of the row (pixel j / 3, channel j % 3): every load of the wave is one contiguous
    // 64-element run (a thread per PIXEL read its 3 values at a 24-byte stride, three passes over the same cache lines).  Per element
    // the additions are still s = 0, 1, 2, ... in order.
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid == 0 && counters && s_begin + s_count >= ns) counters[1] = n_valid_pixels; // metrics total-pixels, core.clj:47
    if (gid >= (long long)n_local_tiles * 64) return;
    const int tile_local = (int)(gid >> 6), l = (int)(gid & 63);
    const int gtile = tile_ids[tile_local];
    const int tx = (gtile % tiles_x) * RTMI_TILE, ty = (gtile / tiles_x) * RTMI_TILE;
    R acc[3];
    bool valid[3];
    const size_t tile_base = (size_t)tile_local * 192;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int p = fold_pixel<DEFER>(l, k); // pixel of the tile this element belongs to
        const int x = tx + (p & 7), y = ty + (p >> 3);
        valid[k] = x >= rx0 && x < rx1 && y >= ry0 && y < ry1;
        acc[k] = (valid[k] && s_begin > 0) ? accum[tile_base + fold_elem<DEFER>(l, k)] : R(0);
    }
    if constexpr (DEFER) {
        const GradientU<R> gu = gradient_rec_u<R>(grad, R(0.5)); // the lerps along u read the material only: once per thread
        const R *rec = samples + ((size_t)tile_local * s_count * 64 + l) * 4;
        for (int s = 0; s < s_count; ++s, rec += 256) {
            R v[3];
            fold_record4<R>(rec, gu, valid[0], v);
            if (s_begin + s == 0) { acc[0] = v[0]; acc[1] = v[1]; acc[2] = v[2]; }
            else { acc[0] = acc[0] + v[0]; acc[1] = acc[1] + v[1]; acc[2] = acc[2] + v[2]; }
        }
    } else {
    const R *row = samples + (size_t)tile_local * s_count * 192 + l;
    for (int s = 0; s < s_count; ++s, row += 192) {
        const R v0 = row[0], v1 = row[64], v2 = row[128];
        if (s_begin + s == 0) { acc[0] = v0; acc[1] = v1; acc[2] = v2; } // the fold starts FROM the first sample (not 0 + first)
        else { acc[0] = acc[0] + v0; acc[1] = acc[1] + v1; acc[2] = acc[2] + v2; }
    }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const size_t o = tile_base + fold_elem<DEFER>(l, k);
        if (s_begin + s_count < ns) accum[o] = valid[k] ? acc[k] : R(0);
        else tiles_linear[o] = valid[k] ? (double)(acc[k] * (R(1.0) / (R)ns)) : 0.0;
    }
}

// core.clj:54-56 + the y-flipped store of core.clj:105-106 (tiles already hold output rows).
// gathered[r][k][64][3]: rank r's k-th tile is global tile r + k*world.
template <typename R>
__global__ void __launch_bounds__(kBlock) assemble_kernel(const double *__restrict__ gathered, int world, size_t rank_stride, int tiles_x,
                                                          int nx, int ny, double *__restrict__ out_linear, unsigned char *__restrict__ out_rgb8) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)nx * ny) return;
    const int x = (int)(gid % nx), y = (int)(gid / nx);
    const int gtile = (y / RTMI_TILE) * tiles_x + (x / RTMI_TILE);
    const int r = gtile % world, k = gtile / world;
    const int l = (y % RTMI_TILE) * RTMI_TILE + (x % RTMI_TILE);
    const double *p = gathered + (size_t)r * rank_stride + ((size_t)k * 64 + l) * 3; // rank_stride: doubles per rank record
    for (int c = 0; c < 3; ++c) {
        const double m = p[c];
        if (out_linear) out_linear[gid * 3 + c] = m;
        if (out_rgb8) {
            const R q = Real<R>::sqrt_((R)m) * R(255.99);
            // (int (min 255.99 q)): clojure.core/min propagates NaN and (int NaN) = 0
            unsigned char o = 0;
            if (q == q) { const R mq = q < R(255.99) ? q : R(255.99); o = (unsigned char)(int)mq; }
            out_rgb8[gid * 3 + c] = o;
        }
    }
}

// The same for a rectangular window of tiles [tx0, tx0+wtx) x [ty0, ...) rendered for the output region [x0, x0+w) x [y0, y0+h):
// tiles[k][64][3], k row-major over the window; writes the dense w x h region.
template <typename R>
__global__ void __launch_bounds__(kBlock) assemble_region_kernel(const double *__restrict__ tiles, int tx0, int ty0, int wtx, int x0, int y0, int w, int h,
                                                                 double *__restrict__ out_linear, unsigned char *__restrict__ out_rgb8) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)w * h) return;
    const int x = x0 + (int)(gid % w), y = y0 + (int)(gid / w);
    const int k = (y / RTMI_TILE - ty0) * wtx + (x / RTMI_TILE - tx0);
    const int l = (y % RTMI_TILE) * RTMI_TILE + (x % RTMI_TILE);
    const double *p = tiles + ((size_t)k * 64 + l) * 3;
    for (int c = 0; c < 3; ++c) {
        const double m = p[c];
        if (out_linear) out_linear[gid * 3 + c] = m;
        if (out_rgb8) {
            const R q = Real<R>::sqrt_((R)m) * R(255.99);
            unsigned char o = 0;
            if (q == q) { const R mq = q < R(255.99) ? q : R(255.99); o = (unsigned char)(int)mq; }
            out_rgb8[gid * 3 + c] = o;
        }
    }
}

// multi-device render: every rank's record ends with its two metrics counters; out = their sums
__global__ void sum_counters_kernel(const u64 *gathered, int world, size_t rank_stride_u64, size_t off_u64, u64 *out) {
    if (threadIdx.x < 2) {
        u64 acc = 0;
        for (int r = 0; r < world; ++r) acc += gathered[(size_t)r * rank_stride_u64 + off_u64 + threadIdx.x];
        out[threadIdx.x] = acc;
    }
}

// ---- probe kernels (one protocol call per thread; same device functions as trace_kernel) -------------
template <typename R> __device__ inline void load_ray(const double *q, Path<R> &P) {
    P.ox = (R)q[0]; P.oy = (R)q[1]; P.oz = (R)q[2]; P.dx = (R)q[3]; P.dy = (R)q[4]; P.dz = (R)q[5]; P.time = (R)q[6];
    P.ar = P.ag = P.ab = R(1); seed_stream(P, 0ull, 0u); P.depth = 0;
}

template <typename R, int VARIANT, bool EXT = false, int MSEQ = 0>
__global__ void __launch_bounds__(kBlock) probe_hit_kernel(ScenePtr scp, int prims_per_tile, int n_ptiles, int n, const double *rays, double tmin, double tmax, double *out) {
    SceneRef sc = *scp;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Prim4<R> *lds = reinterpret_cast<Prim4<R> *>(smem);
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = k < n;
    Path<R> P;
    load_ray<R>(rays + (size_t)(active ? k : 0) * 7, P);
    R best_t; int best_i;
    intersect_world<R, true, VARIANT, EXT, false, false, MSEQ>(sc, lds, prims_per_tile, n_ptiles, P, active, (R)tmin, (R)tmax, best_t, best_i);
    if (!active) return;
    double *o = out + (size_t)k * 11;
    for (int c = 0; c < 11; ++c) o[c] = 0.0;
    if (best_i < 0) return;
    HitRec<R> h;
    resolve_any<R, EXT>(sc, P, best_t, best_i, h);
    o[0] = 1.0; o[1] = h.orig; o[2] = h.t; o[3] = h.px; o[4] = h.py; o[5] = h.pz;
    o[6] = h.nx; o[7] = h.ny; o[8] = h.nz; o[9] = h.u; o[10] = h.v;
}

template <typename R, int VARIANT, bool EXT = false, int MSEQ = 0>
__global__ void __launch_bounds__(kBlock) probe_paths_kernel(ScenePtr scp, int prims_per_tile, int n_ptiles, int n, const double *rays, const u64 *keys, u64 ctr0,
                                                             int depth, double *out_rgb, u64 *out_nseg, double *log, int max_seg, int *out_nlog) {
    SceneRef sc = *scp;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Prim4<R> *lds = reinterpret_cast<Prim4<R> *>(smem);
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    bool alive = k < n;
    Path<R> P;
    load_ray<R>(rays + (size_t)(alive ? k : 0) * 7, P);
    seed_stream(P, alive ? keys[k] : 0ull, (unsigned)ctr0); P.depth = depth;
    SegLog lg = {log ? log + (size_t)(alive ? k : 0) * max_seg * RTMI_SEG_REC : nullptr, max_seg, 0};
    u64 nseg = 0;
    const R tmin = R(0.001), tmax = Real<R>::tmax();
    R rgb[3] = {R(0), R(0), R(0)};
    while (__syncthreads_or(alive ? 1 : 0)) {
        R best_t; int best_i;
        intersect_world<R, true, VARIANT, EXT, false, false, MSEQ>(sc, lds, prims_per_tile, n_ptiles, P, alive, tmin, tmax, best_t, best_i);
        if (alive) {
            ++nseg;
            R emit[3];
            alive = shade_segment<R, EXT>(sc, P, best_t, best_i, log ? &lg : nullptr, emit);
            if (!alive) { rgb[0] = emit[0]; rgb[1] = emit[1]; rgb[2] = emit[2]; }
        }
    }
    if (k < n) {
        out_rgb[3 * k] = rgb[0]; out_rgb[3 * k + 1] = rgb[1]; out_rgb[3 * k + 2] = rgb[2];
        if (out_nseg) out_nseg[k] = nseg;
        if (out_nlog) out_nlog[k] = lg.n;
    }
}

template <typename R> __global__ void probe_camera_kernel(ScenePtr scp, int n, const double *uv, const u64 *keys, double *out) {
    SceneRef sc = *scp;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    Path<R> P;
    seed_stream(P, keys[k], 0u); P.depth = 0;
    get_ray<R>(sc, (R)uv[2 * k], (R)uv[2 * k + 1], P);
    double *o = out + (size_t)k * 8;
    o[0] = P.ox; o[1] = P.oy; o[2] = P.oz; o[3] = P.dx; o[4] = P.dy; o[5] = P.dz; o[6] = P.time; o[7] = (double)P.ctr;
}

template <typename R, bool F4 = false> __global__ void probe_texture_kernel(ScenePtr scp, int tex, int n, const double *uvp, double *out) {
    SceneRef sc = *scp;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double *q = uvp + (size_t)k * 5;
    R r, g, b;
    tex_sample<R, F4>(sc, tex, (R)q[0], (R)q[1], (R)q[2], (R)q[3], (R)q[4], r, g, b);
    out[3 * k] = r; out[3 * k + 1] = g; out[3 * k + 2] = b;
}

// Shader.scatter (shader.clj) on an explicit hit record {p, normal, u, v}: the same scatter_emit the render kernel runs.
template <typename R, bool F4 = false>
__global__ void probe_scatter_kernel(ScenePtr scp, int mat, int n, const double *rays, const double *hits, const u64 *keys, double *out) {
    SceneRef sc = *scp;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    Path<R> P;
    load_ray<R>(rays + (size_t)k * 7, P);
    seed_stream(P, keys[k], 0u); P.depth = 1;
    const double *hq = hits + (size_t)k * 8;
    HitRec<R> h;
    h.t = R(0); h.px = (R)hq[0]; h.py = (R)hq[1]; h.pz = (R)hq[2]; h.nx = (R)hq[3]; h.ny = (R)hq[4]; h.nz = (R)hq[5];
    h.u = (R)hq[6]; h.v = (R)hq[7]; h.orig = -1; h.kind = RTMI_PRIM_SPHERE; h.mat = mat;
    R att[3] = {R(0), R(0), R(0)}, emit[3];
    const bool scat = scatter_emit<R, F4>(sc, P, h, att, emit);
    double *o = out + (size_t)k * 9;
    o[0] = scat ? 1.0 : 0.0;
    o[1] = scat ? P.dx : 0; o[2] = scat ? P.dy : 0; o[3] = scat ? P.dz : 0;
    o[4] = scat ? att[0] : 0; o[5] = scat ? att[1] : 0; o[6] = scat ? att[2] : 0;
    o[7] = scat ? P.time : 0; o[8] = (double)P.ctr;
}

template <typename R> __global__ void probe_rng_kernel(u64 key, u64 d0, int n, u64 *bits, double *real) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const u64 z = draw_bits(key, d0 + (u64)k);
    bits[k] = z;
    real[k] = (double)Real<R>::uniform(z);
}

__global__ void probe_arith_kernel(int n, const double *abc, double *out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double a = abc[3 * k], b = abc[3 * k + 1], c = abc[3 * k + 2];
    out[3 * k] = a / b;
    out[3 * k + 1] = ::sqrt(::fabs(a));
    out[3 * k + 2] = a * b + c; // must stay unfused (-ffp-contract=off)
}

} // namespace

// =====================================================================================================
// host side: C-ABI
// =====================================================================================================
#include "scene_build.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail(RTMI_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// the multi-device entries switch the calling thread's current device; hosts that track it themselves (PyTorch) get it back
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return RTMI_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        if (hipMalloc(&p, need) != hipSuccess) { p = nullptr; return fail(RTMI_E_NOMEM, "hipMalloc(%zu bytes) failed", need); }
        bytes = need;
        return RTMI_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

// ---- progressive and adaptive frame kernels (rtmi_render_progressive*, rtmi_render_adaptive*) ----------------------------------------------------
// The frame's state is tile-major like c->accum: element l + 64 k of local tile t (pixel (l + 64 k) / 3 of the tile, channel (l + 64 k) % 3) sits at
// t * 192 + l + 64 k in three arrays: the running sum of the samples in R (what reduce_kernel keeps between passes), and, in double whatever R is,
// Welford's running mean and M2 of the same samples (the noise estimate; the image never reads them).
// An adaptive call traces only the frame's active tiles.  The active list is two parallel arrays in ascending tile order: act_tiles[i] = global tile
// (what the trace kernel takes as tile_ids, so sample-buffer tile i holds entry i's samples) and act_slots[i] = the tile's local tile number, i.e.
// where its state sits (slot * 192) and what the resolve indexes.  n_t[slot] = samples the tile holds.

// what the retiring fold takes beside the uniform one's arguments (an empty one for the uniform fold, which reads none of it)
struct FoldRetire {
    const int *act_slots = nullptr;
    int last = 0; // the call's last pass: decide
    double eps = 0.0;
    int *keep = nullptr, *n_t = nullptr;
};

// One pass of the sample buffer, samples [s_begin, s_begin + s_count), folded into the state: the sums with reduce_kernel's fold (same order, the
// first sample of the frame is the start value), the noise state with Welford's update.  The wave of entry i of `tiles` folds sample-buffer tile i;
// lane l owns elements l, l + 64, l + 128 of the tile's row, so every load is contiguous.  Elements outside the region keep 0.
// RETIRE = false (a progressive call): `tiles` is the render's tile list and entry i's state sits at i * 192.
// RETIRE = true (an adaptive call): `tiles` is the active list and the state sits at rt.act_slots[i] * 192, same element ownership, same arithmetic.
// On the call's last pass (rt.last) the wave also decides: k = s_begin + s_count, the tile stays active (keep[i] = 1) if k < 2 or any element of a
// valid pixel fails se <= eps, se = sqrt((M2 / (k - 1)) / k) as the resolve computes it, on the M2 in registers (a NaN fails); n_t[slot] = k.
// DEFER: as reduce_kernel's -- 4-real records, a lane owns a pixel; the state's layout and every element's arithmetic are the same.
template <typename R, bool RETIRE, bool DEFER = false>
__global__ void __launch_bounds__(kBlock) frame_fold_kernel(const R *__restrict__ samples, R *__restrict__ sums, double *__restrict__ mean,
                                                            double *__restrict__ m2, const int *__restrict__ tiles, int tiles_x, int n_entries, int s_begin,
                                                            int s_count, u64 *counters, u64 n_valid_pixels, int rx0, int ry0, int rx1, int ry1, FoldRetire rt,
                                                            const double *__restrict__ grad) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid == 0) counters[1] = n_valid_pixels; // metrics total-pixels, core.clj:47
    if (gid >= (long long)n_entries * 64) return; // (whole waves: kBlock is a multiple of 64)
    const int entry = (int)(gid >> 6), l = (int)(gid & 63);
    const int gtile = tiles[entry];
    int slot = entry;
    if constexpr (RETIRE) slot = rt.act_slots[entry];
    const int tx = (gtile % tiles_x) * RTMI_TILE, ty = (gtile / tiles_x) * RTMI_TILE;
    R acc[3];
    double mu[3], q[3];
    bool valid[3];
    const size_t tile_base = (size_t)slot * 192;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int p = fold_pixel<DEFER>(l, k);
        const int x = tx + (p & 7), y = ty + (p >> 3);
        valid[k] = x >= rx0 && x < rx1 && y >= ry0 && y < ry1;
        const bool carry = valid[k] && s_begin > 0;
        const size_t o = tile_base + fold_elem<DEFER>(l, k);
        acc[k] = carry ? sums[o] : R(0);
        mu[k] = carry ? mean[o] : 0.0;
        q[k] = carry ? m2[o] : 0.0;
    }
    GradientU<R> gu = {};
    if constexpr (DEFER) gu = gradient_rec_u<R>(grad, R(0.5)); // the lerps along u read the material only: once per thread
    const R *row = DEFER ? samples + ((size_t)entry * s_count * 64 + l) * 4 : samples + (size_t)entry * s_count * 192 + l;
    for (int s = 0; s < s_count; ++s, row += DEFER ? 256 : 192) {
        R v[3];
        if constexpr (DEFER) fold_record4<R>(row, gu, valid[0], v);
        else { v[0] = row[0]; v[1] = row[64]; v[2] = row[128]; }
        if (s_begin + s == 0) { // the fold starts FROM the first sample (not 0 + first)
#pragma unroll
            for (int k = 0; k < 3; ++k) { acc[k] = v[k]; mu[k] = (double)v[k]; q[k] = 0.0; }
        } else {
            const double n = (double)(s_begin + s + 1);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                acc[k] = acc[k] + v[k];
                const double x = (double)v[k], d = x - mu[k];
                mu[k] = mu[k] + d / n;
                q[k] = q[k] + d * (x - mu[k]); // >= 0 up to rounding; exactly 0 while every sample is equal
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const size_t o = tile_base + fold_elem<DEFER>(l, k);
        sums[o] = valid[k] ? acc[k] : R(0);
        mean[o] = valid[k] ? mu[k] : 0.0;
        m2[o] = valid[k] ? q[k] : 0.0;
    }
    if constexpr (RETIRE) {
        if (!rt.last) return;
        const int kk = s_begin + s_count;
        bool noisy = false;
        if (kk > 1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double se = ::sqrt((q[k] / (double)(kk - 1)) / (double)kk); // pixel_estimate's expression
                noisy = noisy || (valid[k] && !(se <= rt.eps));
            }
        }
        const u64 any = __ballot(noisy);
        if (l == 0) { rt.keep[entry] = (kk < 2 || any != 0ull) ? 1 : 0; rt.n_t[slot] = kk; }
    }
}

// What the state says about one pixel after k samples: m = the three means as reduce_kernel's last pass computes them, sums * (R(1) / R(k)),
// widened to double; err = the largest of the three channels' standard errors of the mean, sqrt((M2 / (k - 1)) / k) (+inf for k <= 1; a NaN
// standard error does not replace the running maximum).  e = the element index of the pixel's first channel.
struct PixelEstimate { double m[3], err; int k; };
template <typename R>
__device__ inline PixelEstimate pixel_estimate(const R *__restrict__ sums, const double *__restrict__ m2, size_t e, int k) {
    PixelEstimate p;
    p.k = k;
    p.err = k > 1 ? 0.0 : INFINITY;
    for (int c = 0; c < 3; ++c) {
        p.m[c] = (double)(sums[e + c] * (R(1.0) / (R)k)); // reduce_kernel's last pass
        if (k > 1) {
            const double se = ::sqrt((m2[e + c] / (double)(k - 1)) / (double)k);
            p.err = se > p.err ? se : p.err;
        }
    }
    return p;
}

// The 8-bit quantiser of a linear mean, in double for both precisions: the one copy below the kernel section.  assemble_kernel and
// assemble_region_kernel above keep their own (their text is part of the hashed kernel section); test_gpu_frame_exact.py pins all copies
// against each other.
__device__ inline unsigned char quantise8(double m) {
    const double q = Real<double>::sqrt_(m) * 255.99;
    unsigned char o = 0;
    if (q == q) { const double mq = q < 255.99 ? q : 255.99; o = (unsigned char)(int)mq; }
    return o;
}

// The state -> the dense region [x0, x0 + w) x [y0, y0 + h) of the frame (its local tiles are the window [tx0, tx0 + wtx) x ..., row-major): per pixel
// pixel_estimate with k = n_t[t] samples behind every pixel of local tile t (n_t = null: a uniform frame, k_uniform everywhere).  out_linear = the
// mean, out_rgb8 = quantise8 of it, out_stderr = the error, out_samples = k.  Any output may be null.
template <typename R>
__global__ void __launch_bounds__(kBlock) frame_resolve_kernel(const R *__restrict__ sums, const double *__restrict__ m2, const int *__restrict__ n_t,
                                                               int k_uniform, int tx0, int ty0, int wtx, int x0, int y0, int w, int h,
                                                               double *__restrict__ out_linear, unsigned char *__restrict__ out_rgb8,
                                                               double *__restrict__ out_stderr, int *__restrict__ out_samples) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)w * h) return;
    const int x = x0 + (int)(gid % w), y = y0 + (int)(gid / w);
    const int t = (y / RTMI_TILE - ty0) * wtx + (x / RTMI_TILE - tx0);
    const int l = (y % RTMI_TILE) * RTMI_TILE + (x % RTMI_TILE);
    const PixelEstimate p = pixel_estimate(sums, m2, ((size_t)t * 64 + l) * 3, n_t ? n_t[t] : k_uniform);
    for (int c = 0; c < 3; ++c) {
        if (out_linear) out_linear[gid * 3 + c] = p.m[c];
        if (out_rgb8) out_rgb8[gid * 3 + c] = quantise8(p.m[c]);
    }
    if (out_stderr) out_stderr[gid] = p.err;
    if (out_samples) out_samples[gid] = p.k;
}

// Ordered compaction of the active list, one workgroup of kCompactBlock threads walking the n entries in strides of its size: entry i survives if
// keep[i] != 0 (keep = null: all survive) and goes to position (survivors before i), so ascending tile order is kept and the result does not depend
// on timing: ballot + popcount give a lane its rank within the wave, an LDS table of the waves' counts the wave's offset within the stride, a
// register the running total.  in_slots = null: the identity (the start of a frame: in_tiles = the render's tile list; init_n_t >= 0 then also
// sets n_t[i]).  meta = {survivors, their pixels inside the image and the region}; ints suffice, a frame has at most 2^30 pixels.
constexpr int kCompactBlock = 1024;
__global__ void __launch_bounds__(kCompactBlock) adaptive_compact_kernel(const int *__restrict__ keep, const int *__restrict__ in_tiles,
                                                                         const int *__restrict__ in_slots, int n, int *__restrict__ out_tiles,
                                                                         int *__restrict__ out_slots, int *__restrict__ meta, int init_n_t,
                                                                         int *__restrict__ n_t, int tiles_x, int rx0, int ry0, int rx1, int ry1) {
    __shared__ int wave_count[kCompactBlock / 64];
    __shared__ int wave_pixels[kCompactBlock / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0, pixels = 0;
    for (int i0 = 0; i0 < n; i0 += kCompactBlock) {
        const int i = i0 + tid;
        const bool in = i < n;
        const bool live = in && (!keep || keep[i] != 0);
        const u64 mask = __ballot(live);
        const int rank = (int)__popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_count[wave] = (int)__popcll(mask);
        __syncthreads();
        int offset = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kCompactBlock / 64; ++w) {
            const int cw = wave_count[w];
            offset += w < wave ? cw : 0;
            total += cw;
        }
        if (live) {
            const int g = in_tiles[i], slot = in_slots ? in_slots[i] : i;
            const int o = base + offset + rank;
            out_tiles[o] = g;
            out_slots[o] = slot;
            const int px0 = (g % tiles_x) * RTMI_TILE, py0 = (g / tiles_x) * RTMI_TILE;
            const int ax0 = max(px0, rx0), ay0 = max(py0, ry0), ax1 = min(px0 + RTMI_TILE, rx1), ay1 = min(py0 + RTMI_TILE, ry1);
            pixels += (ax1 > ax0 && ay1 > ay0) ? (ax1 - ax0) * (ay1 - ay0) : 0;
        }
        if (in && init_n_t >= 0) n_t[i] = init_n_t;
        base += total;
        __syncthreads(); // wave_count is rewritten by the next stride
    }
    for (int d = 32; d > 0; d >>= 1) pixels += __shfl_down(pixels, d, 64);
    if (lane == 0) wave_pixels[wave] = pixels;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
        for (int w = 0; w < kCompactBlock / 64; ++w) sum += wave_pixels[w];
        meta[0] = base;
        meta[1] = sum;
    }
}

// rtmi_adaptive_retire*: the decision of the retiring frame_fold_kernel's last pass taken on a noise map the caller supplies.  One wave per entry of the active
// list, lane l = pixel l of the entry's 8x8 tile: the wave reads eight 64-byte row segments of the whole-frame map [ny][nx] at the tile's place in the
// IMAGE (act_tiles: the global tile; act_slots, the tile's place in the frame's state, is not needed here), only where the pixel lies inside the
// region clipped to the image.  keep[entry] = 1 if any such pixel fails noise <= eps (a NaN fails).  adaptive_compact_kernel follows.
__global__ void __launch_bounds__(kBlock) adaptive_retire_kernel(const double *__restrict__ noise, const int *__restrict__ act_tiles, int n_active,
                                                                 int tiles_x, int nx, int rx0, int ry0, int rx1, int ry1, double eps,
                                                                 int *__restrict__ keep) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n_active * 64) return; // (whole waves: kBlock is a multiple of 64)
    const int entry = (int)(gid >> 6), l = (int)(gid & 63);
    const int gtile = act_tiles[entry];
    const int x = (gtile % tiles_x) * RTMI_TILE + (l & 7), y = (gtile / tiles_x) * RTMI_TILE + (l >> 3);
    const bool valid = x >= rx0 && x < rx1 && y >= ry0 && y < ry1; // rx1 <= nx, ry1 <= ny: the load below stays inside the map
    bool noisy = false;
    if (valid) {
        const double v = noise[(size_t)y * (size_t)nx + (size_t)x];
        noisy = !(v <= eps);
    }
    const u64 any = __ballot(noisy);
    if (l == 0) keep[entry] = any != 0ull ? 1 : 0;
}

// ---- dealt progressive frames (rtmi_render_adaptive_tiles_device, rtmi_assemble_progressive_device, rtmi_render_multi_adaptive*) ------------------
// The frame's local tiles are the dealt tiles first, first + stride, ...: local slot t holds global tile first + t * stride, so no rectangular window
// describes them.  The resolve therefore writes tile RECORDS, rec[t][64][RTMI_PROG_REC]: pixel_estimate's three means, its error and its k, the
// values frame_resolve_kernel writes per pixel, in tile order, the layout a gather moves.
// n_t = null: a uniform frame, every tile holds k samples.  One thread per pixel of the n_slots record slots; slots past the frame's n_local tiles
// (the padding of a gathered record) and pixels outside the image hold five zeros.
template <typename R>
__global__ void __launch_bounds__(kBlock) progressive_record_kernel(const R *__restrict__ sums, const double *__restrict__ m2, const int *__restrict__ n_t,
                                                                    int k_uniform, int first, int stride, int tiles_x, int nx, int ny, int n_local,
                                                                    int n_slots, double *__restrict__ rec) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n_slots * 64) return;
    const int t = (int)(gid >> 6), l = (int)(gid & 63);
    double *o = rec + (size_t)gid * RTMI_PROG_REC;
    bool inside = false;
    if (t < n_local) {
        const long long gtile = (long long)first + (long long)t * stride; // < tiles of the frame: t < n_local
        const int x = (int)(gtile % tiles_x) * RTMI_TILE + (l & 7), y = (int)(gtile / tiles_x) * RTMI_TILE + (l >> 3);
        inside = x < nx && y < ny;
    }
    if (!inside) {
#pragma unroll
        for (int c = 0; c < RTMI_PROG_REC; ++c) o[c] = 0.0;
        return;
    }
    const PixelEstimate p = pixel_estimate(sums, m2, (size_t)gid * 3, n_t ? n_t[t] : k_uniform);
    for (int c = 0; c < 3; ++c) o[c] = p.m[c];
    o[3] = p.err;
    o[4] = (double)p.k;
}

// gathered[r][k][64][RTMI_PROG_REC] (rank r's k-th tile is global tile r + k * world; rank_stride = doubles per rank record) -> the dense frame:
// assemble_kernel<double> for the mean (quantise8), the standard error and the sample count beside it.  Any output may be null.
__global__ void __launch_bounds__(kBlock) assemble_progressive_kernel(const double *__restrict__ gathered, int world, size_t rank_stride, int tiles_x,
                                                                      int nx, int ny, double *__restrict__ out_linear, unsigned char *__restrict__ out_rgb8,
                                                                      double *__restrict__ out_stderr, int *__restrict__ out_samples) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)nx * ny) return;
    const int x = (int)(gid % nx), y = (int)(gid / nx);
    const int gtile = (y / RTMI_TILE) * tiles_x + (x / RTMI_TILE);
    const int r = gtile % world, k = gtile / world;
    const int l = (y % RTMI_TILE) * RTMI_TILE + (x % RTMI_TILE);
    const double *p = gathered + (size_t)r * rank_stride + ((size_t)k * 64 + l) * RTMI_PROG_REC;
    for (int c = 0; c < 3; ++c) {
        const double m = p[c];
        if (out_linear) out_linear[gid * 3 + c] = m;
        if (out_rgb8) out_rgb8[gid * 3 + c] = quantise8(m);
    }
    if (out_stderr) out_stderr[gid] = p[3];
    if (out_samples) out_samples[gid] = (int)p[4];
}

// ---- first-hit feature pass (rtmi_render_features*) -------------------------------------------------------------------------------------------
// One wave per 8x8 tile of the window of tiles that covers the region, one lane per pixel, four waves per workgroup (the LDS stack columns of the
// probe kernels: column = threadIdx.x).  Lane l loops over the feature samples s = 0 .. na-1 of its pixel: the first segment of the path render
// sample s traces -- start_sample (same key, jitter and camera draws), intersect_world with t-min 0.001 (media draw from the sample's stream as in
// the render), resolve_any with both uv coordinates, tex_sample of the material's texture -- and folds the eight values into running sums in
// registers, in sample order, starting FROM sample 0.  No sample buffer, no reduction pass: HBM sees the 64 bytes per pixel of the result.
struct FeatureParams {
    int nx, ny, na;
    u64 seed;
    int tx0, ty0, wtx, n_tiles; // the window of tiles, row-major
    int rx0, ry0, rx1, ry1;     // output region (row 0 = top)
    double *out;                // [ry1 - ry0][rx1 - rx0][8]
    u64 *counters;              // [0] += feature rays, [1] += pixels
};

template <typename R, int VARIANT, bool EXT = false, int MSEQ = 0>
__global__ void __launch_bounds__(kBlock) feature_kernel(ScenePtr scp, FeatureParams fp) {
    static_assert(VARIANT >= SCAN_SGPR, "the LDS-staged scans need workgroup barriers: the feature pass does not run them");
    SceneRef sc = *scp;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Prim4<R> *lds = reinterpret_cast<Prim4<R> *>(smem);
    const int lane = threadIdx.x & 63;
    const int tile = (int)((blockIdx.x * (unsigned)kBlock + threadIdx.x) >> 6); // wave-uniform
    const bool in_grid = tile < fp.n_tiles;
    const int tcol = in_grid ? tile % fp.wtx : 0, trow = in_grid ? tile / fp.wtx : 0;
    const int x = (fp.tx0 + tcol) * RTMI_TILE + (lane & 7), y = (fp.ty0 + trow) * RTMI_TILE + (lane >> 3);
    const bool active = in_grid && x >= fp.rx0 && x < fp.rx1 && y >= fp.ry0 && y < fp.ry1;
    TraceParams tp;
    tp.seed = fp.seed; tp.nx = fp.nx; tp.ny = fp.ny; tp.depth = 0;
    const R tmin = R(0.001), tmax = Real<R>::tmax();
    R acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = R(0);
    for (int s = 0; s < fp.na; ++s) {
        Path<R> P;
        P.ox = P.oy = P.oz = P.dx = P.dy = P.dz = P.time = R(0);
        P.ar = P.ag = P.ab = R(0);
        seed_stream(P, 0ull, 0u); P.depth = 0;
        if (active) start_sample<R>(sc, tp, x, fp.ny - 1 - y, s, P); // j = ny-1-y (core.clj:105)
        const R ox = P.ox, oy = P.oy, oz = P.oz;
        R best_t; int best_i;
        intersect_world<R, false, VARIANT, EXT, false, false, MSEQ>(sc, lds, 0, 1, P, active, tmin, tmax, best_t, best_i);
        R f[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) f[c] = R(0);
        if (active && best_i >= 0) {
            HitRec<R> h;
            resolve_any<R, EXT>(sc, P, best_t, best_i, h, true);
            const int mk = sc.mat_kind[h.mat];
            if (mk == RTMI_MAT_DIELECTRIC) f[0] = f[1] = f[2] = R(1);
            else tex_sample<R, EXT>(sc, sc.mat_tex[h.mat], h.u, h.v, h.px, h.py, h.pz, f[0], f[1], f[2]);
            f[3] = h.nx; f[4] = h.ny; f[5] = h.nz;
            const R ex = h.px - ox, ey = h.py - oy, ez = h.pz - oz;
            f[6] = Real<R>::sqrt_(dot3(ex, ey, ez, ex, ey, ez));
            f[7] = R(1);
        }
        if (s == 0) { // the fold starts FROM the first sample (not 0 + first)
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = f[c];
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = acc[c] + f[c];
        }
    }
    const u64 live = __ballot(active);
    if (lane == 0 && live) {
        atomicAdd(fp.counters, (u64)__popcll(live) * (u64)fp.na);
        atomicAdd(fp.counters + 1, (u64)__popcll(live));
    }
    if (!active) return;
    const R inv = R(1.0) / (R)fp.na; // the frame's mean: sum * (1 / n)
    double *o = fp.out + ((size_t)(y - fp.ry0) * (size_t)(fp.rx1 - fp.rx0) + (size_t)(x - fp.rx0)) * 8;
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = (double)(acc[c] * inv);
}

// ---- caller-supplied rays (rtmi_render_rays*) ------------------------------------------------------------------------------------------------
// A work item is one ray = one path.  Persistent waves over one queue, trace_kernel's plain refill loop: a wave claims qblock consecutive items with
// one atomic and deals them to its dead lanes in lane order; a dead lane loads the 7 doubles of its row and its key (or derives it), seeds its
// stream and runs probe_paths_kernel's trip -- intersect_world without time-slicing, so a long segment walks its entry-grid pieces, then
// shade_segment -- next to the live lanes' trips.  The loop is wave-level (no workgroup barrier), hence the scans that need none, as feature_kernel.
// Which lane traces a ray never affects the result: the stream is a function of the ray's key only.  A pass covers rows [row0, row0 + total_items):
// rays, keys and samples are the pass's own (already offset), row0 only enters the derived keys.
struct RaysParams {
    const double *rays;   // [total_items][7]
    const u64 *keys;      // [total_items], or null: sample_key(seed, g, g_first + r) of row row0 + m = g * group + r
    double *samples;      // [total_items][3]
    u64 seed;
    unsigned ctr0;
    int depth;
    unsigned group, g_first, row0;
    unsigned total_items; // <= 2^31 - 64: a claim past the end cannot wrap the queue head
    unsigned qblock;      // items a wave claims per queue access
    unsigned *queue;      // zeroed before the launch
    u64 *counters;        // [0] += segments
    // the frame of a generated source (SRC_CAMERA; never read by the memory source): group g is pixel (g % nx, g / nx), row 0 at the top
    int nx, ny;
    int fixed_rays;       // TraceParams::fixed_rays (read by the wave-wide lens sampler only: RTMI_LIT_WAVE_LENS)
    double *out_camera;   // [total_items][8], or null: origin, direction, time, stream position behind the camera
    // the tile list of SRC_CAMERA_TILES (never read by another source): the pass's own entries, total_items = entries * 64 * group
    const int *tiles;     // [entries]: global 8x8 tile indices, row-major over tiles_x x ceil(ny / 8); an entry outside [0, n_frame_tiles) holds no pixel
    int tiles_x, n_frame_tiles;
};

// Where a lane's ray comes from (the query kernels' sources are described at query_kernel).  SRC_CAMERA, the path kernels' (rtmi_render_lit*): row
// row0 + m is sample g_first + r of pixel g, and the lane builds start_sample's ray in R from the camera the scene holds on the device.
// SRC_CAMERA_TILES (rtmi_render_lit_tiles*): SRC_CAMERA with the pixels taken from a list of 8x8 tiles, THE TILE ORDER of rtmi.h.
enum { SRC_MEMORY = 0, SRC_HEMISPHERE = 1, SRC_TARGETS = 2, SRC_PIXEL = 3, SRC_LIGHT = 4, SRC_CAMERA = 5, SRC_CAMERA_TILES = 6 };

#ifndef RTMI_LIT_WAVE_LENS
#define RTMI_LIT_WAVE_LENS 0 // 1: the refill samples the lens with get_ray_wave, the whole wave helping (A/B; DESIGN.md section 7q: the same bits)
#endif
// The refill of a SRC_CAMERA lane, THE FRAME RULE of rtmi.h: start_sample's operations, so the path goes on in the stream where rtmi_render's does.
// `has`: the lane takes item m; every lane of the wave calls (the refill loop is wave-uniform), the others leave P as it is.
// camera_refill_at: steps 2 - 5 for sample s of pixel (x, j) as item m of the pass; camera_refill: step 1 for the frame's row-major rows in front of it.
template <typename R> __device__ inline void camera_refill_at(SceneRef sc, const RaysParams &rp, bool has, unsigned m, int x, int j, int s, Path<R> &P) {
    const u64 key = sample_key(rp.seed, (u64)j * (u64)rp.nx + (u64)x, (u64)s);
#if RTMI_LIT_WAVE_LENS
    Path<R> Q;
    seed_stream(Q, key, 0u);
    const R u = ((R)(float)x + next_uniform(Q)) / (R)rp.nx;
    const R v = ((R)(float)j + next_uniform(Q)) / (R)rp.ny;
    get_ray_wave<R>(sc, rp.fixed_rays != 0, has, u, v, Q);
    if (has) { P.ox = Q.ox; P.oy = Q.oy; P.oz = Q.oz; P.dx = Q.dx; P.dy = Q.dy; P.dz = Q.dz; P.time = Q.time; P.key = Q.key; P.rs = Q.rs; P.ctr = Q.ctr; }
#else
    if (has) {
        seed_stream(P, key, 0u);
        const R u = ((R)(float)x + next_uniform(P)) / (R)rp.nx;
        const R v = ((R)(float)j + next_uniform(P)) / (R)rp.ny;
        get_ray<R>(sc, u, v, P);
    }
#endif
    if (has) { P.ar = P.ag = P.ab = R(1); P.depth = rp.depth; }
    if (rp.out_camera) { // wave-uniform
        if (has) {
            double *o = rp.out_camera + (size_t)m * 8;
            o[0] = (double)P.ox; o[1] = (double)P.oy; o[2] = (double)P.oz; o[3] = (double)P.dx; o[4] = (double)P.dy; o[5] = (double)P.dz;
            o[6] = (double)P.time; o[7] = (double)P.ctr;
        }
    }
}
template <typename R> __device__ inline void camera_refill(SceneRef sc, const RaysParams &rp, bool has, unsigned m, Path<R> &P) {
    const unsigned row = rp.row0 + m, g = row / rp.group, y = g / (unsigned)rp.nx;
    const int x = (int)(g - y * (unsigned)rp.nx), j = rp.ny - 1 - (int)y, s = (int)(rp.g_first + (row - g * rp.group)); // j = ny-1-y (core.clj:105)
    camera_refill_at<R>(sc, rp, has, m, x, j, s, P);
}

// The refill of a SRC_CAMERA_TILES lane, THE TILE ORDER of rtmi.h: item m of the pass is sample g_first + m % group of local pixel (m / group) % 64 of
// entry m / (64 * group) of the pass's list.  The divisions and the load of the tile index happen here, once per path; the entries of a claimed block
// differ from lane to lane unless 64 * group divides the block, so the index is a per-lane load.  -> the lane took a pixel.  An item whose pixel lies
// outside the image (a partial tile's) leaves +0.0 in its rows of samples and out_camera and its lane dead; an entry outside [0, n_frame_tiles) -- a
// device list is the caller's -- touches nothing at all.
template <typename R> __device__ inline bool tile_refill(SceneRef sc, const RaysParams &rp, bool has, unsigned m, Path<R> &P) {
    const unsigned px = m / rp.group, r = m - px * rp.group, entry = px >> 6, l = px & 63u;
    const int t = has ? rp.tiles[entry] : -1; // entry < the pass's entries: m < total_items
    const bool listed = (unsigned)t < (unsigned)rp.n_frame_tiles;
    const int ty = listed ? t / rp.tiles_x : 0, tx = listed ? t - ty * rp.tiles_x : 0;
    const int x = tx * RTMI_TILE + (int)(l & 7u), y = ty * RTMI_TILE + (int)(l >> 3);
    const bool inside = listed && x < rp.nx && y < rp.ny;
    if (listed && !inside) {
        double *o = rp.samples + (size_t)m * 3;
        o[0] = 0.0; o[1] = 0.0; o[2] = 0.0;
        if (rp.out_camera) {
            double *c = rp.out_camera + (size_t)m * 8;
#pragma unroll
            for (int k = 0; k < 8; ++k) c[k] = 0.0;
        }
    }
    camera_refill_at<R>(sc, rp, inside, m, inside ? x : 0, inside ? rp.ny - 1 - y : 0, (int)(rp.g_first + r), P);
    return inside;
}

template <typename R, int VARIANT, bool EXT = false, int MSEQ = 0, int SRC = SRC_MEMORY>
__global__ void __launch_bounds__(kBlock, EXT ? (MSEQ != 0 ? 3 : RTMI_EXT_MIN_WAVES) : RTMI_MIN_WAVES) rays_kernel(ScenePtr scp, RaysParams rp) {
    static_assert(SRC == SRC_MEMORY || SRC == SRC_CAMERA || SRC == SRC_CAMERA_TILES, "the path kernels read their rays or build the frame's");
    static_assert(VARIANT >= SCAN_SGPR, "the LDS-staged scans need workgroup barriers: the refill loop is per wave");
    SceneRef sc = *scp;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Prim4<R> *lds = reinterpret_cast<Prim4<R> *>(smem);
    const int lane = threadIdx.x & 63;
    const unsigned total_items = rp.total_items;
    unsigned w_cur = 0, w_end = 0; // this wave's claimed range [w_cur, w_end): wave-uniform
    Path<R> P;
    P.ox = P.oy = P.oz = P.dx = P.dy = P.dz = P.time = R(0);
    P.ar = P.ag = P.ab = R(0);
    seed_stream(P, 0ull, 0u); P.depth = 0;
    bool alive = false;
    bool exhausted = (total_items == 0);
    unsigned out_item = 0;
    unsigned nseg = 0;
    const R tmin = R(0.001), tmax = Real<R>::tmax();
    for (;;) {
        while (!exhausted) { // every lane of the wave takes part: the loop conditions are wave-uniform
            const u64 dead = __ballot(!alive);
            if (dead == 0) break;
            if (w_cur == w_end) {
                unsigned base = 0;
                if (lane == 0) base = atomicAdd(rp.queue, rp.qblock);
                base = __builtin_amdgcn_readfirstlane(base);
                if (base >= total_items) { exhausted = true; break; }
                w_cur = base;
                w_end = min(base + rp.qblock, total_items);
            }
            const unsigned avail = w_end - w_cur;
            const unsigned rank = (unsigned)__popcll(dead & ((1ull << lane) - 1ull));
            if constexpr (SRC == SRC_CAMERA) {
                const bool has = !alive && rank < avail;
                const unsigned m = w_cur + (has ? rank : 0u); // < total_items
                camera_refill<R>(sc, rp, has, m, P);
                if (has) { out_item = m; alive = true; }
            } else if constexpr (SRC == SRC_CAMERA_TILES) { // a lane whose item holds no pixel stays dead: the next round of this loop deals it another
                const bool has = !alive && rank < avail;
                const unsigned m = w_cur + (has ? rank : 0u); // < total_items
                if (tile_refill<R>(sc, rp, has, m, P)) { out_item = m; alive = true; }
            } else if (!alive && rank < avail) {
                const unsigned m = w_cur + rank; // < total_items
                load_ray<R>(rp.rays + (size_t)m * 7, P);
                u64 key;
                if (rp.keys) key = rp.keys[m];
                else { const unsigned row = rp.row0 + m, g = row / rp.group; key = sample_key(rp.seed, (u64)g, (u64)rp.g_first + (u64)(row - g * rp.group)); }
                seed_stream(P, key, rp.ctr0); P.depth = rp.depth;
                out_item = m;
                alive = true;
            }
            w_cur += min((unsigned)__popcll(dead), avail);
        }
        if (!__any(alive ? 1 : 0)) break;
        R best_t; int best_i;
        intersect_world<R, true, VARIANT, EXT, false, false, MSEQ>(sc, lds, 0, 1, P, alive, tmin, tmax, best_t, best_i);
        if (alive) {
            ++nseg;
            R emit[3];
            alive = shade_segment<R, EXT>(sc, P, best_t, best_i, nullptr, emit);
            if (!alive) {
                double *out = rp.samples + (size_t)out_item * 3;
                out[0] = (double)emit[0]; out[1] = (double)emit[1]; out[2] = (double)emit[2];
            }
        }
    }
    // segments: wave reduction, one atomic per wave
    unsigned n = nseg;
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off);
    if (lane == 0 && n) atomicAdd(rp.counters, (u64)n);
}

// One lane per group (consecutive lanes, consecutive groups), looping over the group's rows in order: the sums with reduce_kernel's fold in R (the
// first ray of the group is the start value), the noise state with frame_fold_kernel's Welford update in double (restated: that kernel's update is
// part of its body), then pixel_estimate's mean and standard error over count = first + group rays.  state (may be null): the records, read when
// first > 0 and written back; without one first is 0.  samples holds groups [g0, g0 + n_groups) of the call; mean, se and state are the call's.
template <typename R>
__global__ void __launch_bounds__(kBlock) rays_fold_kernel(const double *__restrict__ samples, int g0, int n_groups, int group, int first,
                                                           double *__restrict__ state, double *__restrict__ mean, double *__restrict__ se,
                                                           u64 *counters, u64 n_rays) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid == 0 && counters) counters[1] = n_rays;
    if (gid >= n_groups) return;
    const size_t g = (size_t)g0 + (size_t)gid;
    R acc[3] = {R(0), R(0), R(0)};
    double mu[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
    double *rec = state ? state + g * RTMI_RAYS_REC : nullptr;
    if (rec && first > 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { acc[k] = (R)rec[k]; mu[k] = rec[3 + k]; q[k] = rec[6 + k]; }
    }
    const double *row = samples + (size_t)gid * (size_t)group * 3;
    for (int s = 0; s < group; ++s, row += 3) {
        const R v[3] = {(R)row[0], (R)row[1], (R)row[2]};
        if (first + s == 0) { // the fold starts FROM the first ray (not 0 + first)
#pragma unroll
            for (int k = 0; k < 3; ++k) { acc[k] = v[k]; mu[k] = (double)v[k]; q[k] = 0.0; }
        } else {
            const double n = (double)(first + s + 1);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                acc[k] = acc[k] + v[k];
                const double x = (double)v[k], d = x - mu[k];
                mu[k] = mu[k] + d / n;
                q[k] = q[k] + d * (x - mu[k]);
            }
        }
    }
    const int count = first + group;
    if (rec) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { rec[k] = (double)acc[k]; rec[3 + k] = mu[k]; rec[6 + k] = q[k]; }
        rec[9] = (double)count;
    }
    double err = count > 1 ? 0.0 : INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mean[g * 3 + k] = (double)(acc[k] * (R(1.0) / (R)count));
        if (count > 1) {
            const double e = ::sqrt((q[k] / (double)(count - 1)) / (double)count);
            err = e > err ? e : err;
        }
    }
    se[g] = err;
}

// rtmi_render_lit_tiles*: rays_fold_kernel over a pass of THE TILE ORDER.  One wave per entry of the pass's list, lane l = local pixel l: group
// entry * 64 + l of the pass folds into pixel (x, y) of the whole-frame state, mean and se, and the frame's quantiser runs on the means it wrote (rgb8
// may be null).  A lane outside the image and every lane of an entry outside [0, n_frame_tiles) reads and writes nothing.
template <typename R>
__global__ void __launch_bounds__(kBlock) lit_tiles_fold_kernel(const double *__restrict__ samples, const int *__restrict__ tiles, int n_entries, int group,
                                                                int first, int tiles_x, int n_frame_tiles, int nx, int ny, double *__restrict__ state,
                                                                double *__restrict__ mean, double *__restrict__ se, unsigned char *__restrict__ rgb8) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n_entries * 64) return; // (whole waves: kBlock is a multiple of 64)
    const int entry = (int)(gid >> 6), l = (int)(gid & 63);
    const int t = tiles[entry];
    const bool listed = (unsigned)t < (unsigned)n_frame_tiles;
    const int ty = listed ? t / tiles_x : 0, tx = listed ? t - ty * tiles_x : 0;
    const int x = tx * RTMI_TILE + (l & 7), y = ty * RTMI_TILE + (l >> 3);
    const bool inside = listed && x < nx && y < ny;
    if (!inside) return;
    const size_t g = (size_t)y * (size_t)nx + (size_t)x;
    // rays_fold_kernel's body from here to se[g], expression by expression (that kernel stays as it is for its callers): the bits are its bits
    R acc[3] = {R(0), R(0), R(0)};
    double mu[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
    double *rec = state ? state + g * RTMI_RAYS_REC : nullptr;
    if (rec && first > 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { acc[k] = (R)rec[k]; mu[k] = rec[3 + k]; q[k] = rec[6 + k]; }
    }
    const double *row = samples + (size_t)gid * (size_t)group * 3;
    for (int s = 0; s < group; ++s, row += 3) {
        const R v[3] = {(R)row[0], (R)row[1], (R)row[2]};
        if (first + s == 0) { // the fold starts FROM the first ray (not 0 + first)
#pragma unroll
            for (int k = 0; k < 3; ++k) { acc[k] = v[k]; mu[k] = (double)v[k]; q[k] = 0.0; }
        } else {
            const double n = (double)(first + s + 1);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                acc[k] = acc[k] + v[k];
                const double x = (double)v[k], d = x - mu[k];
                mu[k] = mu[k] + d / n;
                q[k] = q[k] + d * (x - mu[k]);
            }
        }
    }
    const int count = first + group;
    if (rec) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { rec[k] = (double)acc[k]; rec[3 + k] = mu[k]; rec[6 + k] = q[k]; }
        rec[9] = (double)count;
    }
    double err = count > 1 ? 0.0 : INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mean[g * 3 + k] = (double)(acc[k] * (R(1.0) / (R)count));
        if (count > 1) {
            const double e = ::sqrt((q[k] / (double)(count - 1)) / (double)count);
            err = e > err ? e : err;
        }
    }
    se[g] = err;
    if (rgb8) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb8[g * 3 + k] = quantise8(mean[g * 3 + k]);
    }
}

// The rays of a pass of rtmi_render_lit_tiles*: counters[1] += (the pixels of its entries inside the image) * group -- a device list cannot be counted on the
// host, and an atomic per folded tile (32 400 of them at 1920 x 1080, all on one address) cost five times the fold.  One workgroup walks the list in
// strides of its size, as adaptive_compact_kernel does; the passes of a call run in stream order behind the memset that zeroes the counters.
__global__ void __launch_bounds__(kCompactBlock) lit_tiles_count_kernel(const int *__restrict__ tiles, int n_entries, int group, int tiles_x, int n_frame_tiles,
                                                                        int nx, int ny, u64 *counters) {
    __shared__ int wave_pixels[kCompactBlock / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int pixels = 0; // <= 64 * entries / kCompactBlock per thread and <= nx * ny < 2^31 in all
    for (int i = tid; i < n_entries; i += kCompactBlock) {
        const int t = tiles[i];
        if ((unsigned)t < (unsigned)n_frame_tiles) {
            const int ty = t / tiles_x, tx = t - ty * tiles_x;
            pixels += min(RTMI_TILE, nx - tx * RTMI_TILE) * min(RTMI_TILE, ny - ty * RTMI_TILE);
        }
    }
    for (int d = 32; d > 0; d >>= 1) pixels += __shfl_down(pixels, d, 64);
    if (lane == 0) wave_pixels[wave] = pixels;
    __syncthreads();
    if (tid == 0) {
        u64 sum = 0;
        for (int w = 0; w < kCompactBlock / 64; ++w) sum += (u64)wave_pixels[w];
        counters[1] += sum * (u64)group;
    }
}

// rtmi_render_lit*'s 8-bit frame: the frame's quantiser on the fold's means, n = 3 * pixels values
__global__ void __launch_bounds__(kBlock) lit_quantise_kernel(const double *__restrict__ mean, size_t n, unsigned char *__restrict__ out_rgb8) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out_rgb8[i] = quantise8(mean[i]);
}

// rtmi_lit_tiles_records_device: a replica's dealt tiles out of its WHOLE-FRAME planes into progressive_record_kernel's layout, rec[n_slots][64][RTMI_PROG_REC]:
// slot t is global tile first + t * stride, lane l = local pixel l.  The mean and the error are the planes' values as they are, the samples word [9] of the
// pixel's RTMI_RAYS_REC record.  One thread per record pixel, so a wave writes one contiguous 64 * 40 = 2560-byte run; a slot whose tile lies at or past the
// frame's last (the padding of a gathered record) and a pixel outside the image read nothing and hold five zeros.  No tile list is read.
__global__ void __launch_bounds__(kBlock) lit_tiles_record_kernel(const double *__restrict__ state, const double *__restrict__ mean, const double *__restrict__ se,
                                                                  int first, int stride, int tiles_x, int n_frame_tiles, int nx, int ny, int n_slots,
                                                                  double *__restrict__ rec) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n_slots * 64) return;
    const int t = (int)(gid >> 6), l = (int)(gid & 63);
    const long long gtile = (long long)first + (long long)t * stride;
    double v[RTMI_PROG_REC] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (gtile < (long long)n_frame_tiles) {
        const int ty = (int)(gtile / tiles_x), tx = (int)(gtile - (long long)ty * tiles_x);
        const int x = tx * RTMI_TILE + (l & 7), y = ty * RTMI_TILE + (l >> 3);
        if (x < nx && y < ny) {
            const size_t g = (size_t)y * (size_t)nx + (size_t)x;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = mean[g * 3 + c];
            v[3] = se[g];
            v[4] = state[g * RTMI_RAYS_REC + 9];
        }
    }
    double *o = rec + (size_t)gid * RTMI_PROG_REC;
#pragma unroll
    for (int c = 0; c < RTMI_PROG_REC; ++c) o[c] = v[c];
}

// ---- closest-hit and any-hit queries on caller-supplied rays (rtmi_query_hits*, rtmi_query_occluded*) ------------------------------------------------
// A work item is one ray = one hit? of the world (probe_hit_kernel's trip), so every lane is free again after every trip: persistent waves over one queue with
// rays_kernel's claim -- qblock (a multiple of 64) consecutive items per atomic --, of which the wave takes 64 consecutive rays per trip, lane order = row order.
// ANY = false: the record of probe_hit_kernel (resolve_any with every uv) plus the material.  ANY = true: the flag alone, found by the searches that leave at
// the first accepted primitive (intersect_world<..., ANY>); group counts are popcounts over each run of lanes that share a group -- rows are consecutive, so a
// group is one run per wave -- added with one atomic per run.  COUNT (<double, SCAN_BVH, EXT = false> only): the traversal counters of option "count_traversal".
struct QueryParams {
    const double *rays;    // [total_items][7]
    const double *t_range; // [total_items][2], or null: every ray takes tmin, tmax
    const u64 *keys;       // [total_items], or null: every stream is keyed 0
    double tmin, tmax;
    unsigned ctr0;
    unsigned group;        // ANY with count: rays per group
    unsigned total_items;  // <= 2^31 - 64: a claim past the end cannot wrap the queue head
    unsigned qblock;       // items a wave claims per queue access, a multiple of 64
    unsigned *queue;       // zeroed before the launch
    double *hits;          // ANY = false: [total_items][RTMI_HIT_REC]
    unsigned char *occluded; // ANY = true: [total_items], or null
    int *count;            // ANY = true: [ceil(total_items / group)], zeroed before the launch, or null
    u64 *counters;         // [0] += rays, [1] += rays that hit; zeroed before the launch
    u64 *trav;             // COUNT: [0] += AABB tests, [1] += primitive tests
    // generated sources (SRC != SRC_MEMORY; never read by the memory source): the points, what is known of the rays that found them, and the stream
    const double *src_hits;    // [n_points][RTMI_HIT_REC]: rtmi_query_hits' records
    const double *src_view;    // [n_points][7]: the ray that found each point (its direction picks the side, its time is the new ray's), or null
    const double *src_targets; // SRC_TARGETS: [group][3]
    double *out_rays;          // [total_items][7]: the rays as generated (FP64), zeros where a point yields none; or null
    u64 src_seed;              // SRC_HEMISPHERE: the stream of direction k of point g is keyed sample_key(src_seed, g, src_first + k)
    double src_time;           // the rays' time without a view array
    unsigned src_first;
    unsigned src_nx, src_ny;   // the view of SRC_PIXEL and of src_view_camera
    unsigned src_view_camera;  // SRC_HEMISPHERE, no view array: point g is pixel g of the src_nx x src_ny view and its view ray that pixel's centre ray, built again
    // SRC_LIGHT (never read by another source): item m = (g * n_samples + k) * src_n_lights + l of the pass, whose first point is point src_g0 of the call
    const double *src_lights;  // [src_n_lights][kLightRec]: kind, 5 geometry doubles, area, Le.rgb
    double *contrib;           // [total_items][3]: Le * w where the ray was built and is not occluded, else +0.0; or null
    unsigned src_n_lights;
    unsigned src_g0;           // enters the key and the pixel of src_view_camera; src_hits, src_view, out_rays, occluded and contrib are the pass's own
    unsigned src_n_mats;       // src_lambert: a record whose material index is outside [0, src_n_mats) yields no ray
    unsigned src_lambert;      // only points on a RTMI_MAT_LAMBERTIAN material yield rays
};
constexpr int kLightRec = 10;

// Where a lane's ray comes from.  SRC_MEMORY: row m of qp.rays.  The others build it in registers, in FP64 whatever R is, by the rules of rtmi.h
// (rtmi_occlusion_hemisphere, rtmi_occlusion_targets, rtmi_ambient_occlusion): every product, sum and quotient one IEEE operation in the header's order,
// so that numpy restates them bit for bit; the seven doubles then go through load_ray as if they had been read.
// SRC_LIGHT: towards a sampled point of an area light, by the light rule of rtmi.h (rtmi_direct_irradiance); the lane writes the sample's
// contribution before the search and zeroes it behind the search if the ray is occluded.
// (the enum stands above RaysParams: the path kernels' SRC_CAMERA is one of its values)

// pixel m of an nx x ny view, row-major from the top, through its centre from the camera the scene holds on the device (DeviceScene.pixel_centre_rays)
__device__ inline void pixel_centre_ray(SceneRef sc, unsigned m, unsigned nx, unsigned ny, double *q) {
    unsigned long long cam_addr = (unsigned long long)(&sc.cam[0]);
    asm volatile("" : "+s"(cam_addr)); // (as get_ray: the camera's loads stay at their use site)
    const __attribute__((address_space(4))) double *c = (const __attribute__((address_space(4))) double *)cam_addr;
    const unsigned j = m / nx, i = m - j * nx;
    const double u = ((double)i + 0.5) / (double)nx, v = (((double)(ny - 1u) - (double)j) + 0.5) / (double)ny;
    q[0] = c[0]; q[1] = c[1]; q[2] = c[2];
    q[3] = ((c[3] + c[6] * u) + c[9] * v) + (-c[0]);
    q[4] = ((c[4] + c[7] * u) + c[10] * v) + (-c[1]);
    q[5] = ((c[5] + c[8] * u) + c[11] * v) + (-c[2]);
    q[6] = sc.cam_kind == RTMI_CAM_PINHOLE ? 0.0 : c[22];
}

// The ray of item m of a generated source -> q[7]; false: its point yields none (q is zeros).  Every lane of the wave calls (the disk sampler is
// cooperative); a lane past the end of the queue passes in_range = false and m = 0.
template <int SRC> __device__ inline bool generate_ray(SceneRef sc, const QueryParams &qp, bool in_range, unsigned m, double *q) {
    if (SRC == SRC_PIXEL) { pixel_centre_ray(sc, m, qp.src_nx, qp.src_ny, q); return in_range; }
    const double big = __builtin_inf();
    const unsigned g = m / qp.group, k = m - g * qp.group;
    const double *rec = qp.src_hits + (size_t)g * RTMI_HIT_REC;
    const double px = rec[3], py = rec[4], pz = rec[5];
    bool ok = in_range && rec[0] != 0.0 && ::fabs(px) < big && ::fabs(py) < big && ::fabs(pz) < big; // finite: neither inf nor NaN
    double time = qp.src_time, wx = 0.0, wy = 0.0, wz = 0.0;
    bool sided = false;
    if (qp.src_view) { const double *w = qp.src_view + (size_t)g * 7; wx = w[3]; wy = w[4]; wz = w[5]; time = w[6]; sided = true; }
    else if (SRC == SRC_HEMISPHERE && qp.src_view_camera) { double w[7]; pixel_centre_ray(sc, g, qp.src_nx, qp.src_ny, w); wx = w[3]; wy = w[4]; wz = w[5]; time = w[6]; sided = true; }
    double dx, dy, dz;
    if (SRC == SRC_TARGETS) {
        const double *tg = qp.src_targets + (size_t)k * 3;
        dx = tg[0] - px; dy = tg[1] - py; dz = tg[2] - pz;
    } else {
        double nx = rec[6], ny = rec[7], nz = rec[8];
        const double len2 = dot3(nx, ny, nz, nx, ny, nz);
        ok = ok && ::fabs(nx) < big && ::fabs(ny) < big && ::fabs(nz) < big && len2 > 0.0;
        // step 6 before steps 2 - 5 (no operation changes): the wave is still whole here, as the cooperative rounds need it
        Path<double> G; // the generator's own stream; the ray's (what a ConstantMedium draws from) is load_ray's
        seed_stream(G, sample_key(qp.src_seed, (u64)g, (u64)qp.src_first + (u64)k), 0u);
        double x = 0.0, y = 0.0;
        rand_in_unit_disk_wave<double>(G, ok, false, x, y); // Malley: a uniform point of the unit disk, lifted onto the hemisphere
        if (sided && dot3(nx, ny, nz, wx, wy, wz) > 0.0) { nx = -nx; ny = -ny; nz = -nz; } // the normal points away from the viewer: the other side
        const double len = ::sqrt(len2);
        nx = nx / len; ny = ny / len; nz = nz / len;
        double tx, ty, tz; // the frame: the coordinate axis least aligned with the normal, crossed with it
        if (::fabs(nx) < 0.5) { tx = 0.0; ty = -nz; tz = ny; } else { tx = nz; ty = 0.0; tz = -nx; }
        const double tl = ::sqrt(dot3(tx, ty, tz, tx, ty, tz));
        tx = tx / tl; ty = ty / tl; tz = tz / tl;
        const double bx = ny * tz - nz * ty, by = nz * tx - nx * tz, bz = nx * ty - ny * tx;
        const double z = ::sqrt(1.0 - (x * x + y * y));
        dx = (x * tx + y * bx) + z * nx; dy = (x * ty + y * by) + z * ny; dz = (x * tz + y * bz) + z * nz;
    }
    q[0] = ok ? px : 0.0; q[1] = ok ? py : 0.0; q[2] = ok ? pz : 0.0;
    q[3] = ok ? dx : 0.0; q[4] = ok ? dy : 0.0; q[5] = ok ? dz : 0.0; q[6] = ok ? time : 0.0;
    return ok;
}

// SRC_LIGHT: the shadow ray of item m = (g * n_samples + k) * n_lights + l -> q[7] and c[3] = Le * w, w = ((cp cl) / d2^2) area, what the item contributes if
// the ray reaches its light; false: the item yields no ray (q and c are zeros).  Every lane of the wave calls: a sphere light's disk point comes from the
// cooperative sampler, and a wave holds lights of both kinds -- so every lane enters the disk rounds, the sphere lanes with `need`, and the two uniforms of
// a rectangle are read off the key (draws 0 and 1) without a stream.  As in generate_ray the rounds stand before the frame is built (no operation changes).
__device__ inline bool generate_light_ray(SceneRef sc, const QueryParams &qp, bool in_range, unsigned m, double *q, double *c) {
    const double big = __builtin_inf();
    const unsigned nl = qp.src_n_lights;
    const unsigned g = m / qp.group, r = m - g * qp.group, k = r / nl, l = r - k * nl;
    const unsigned gg = qp.src_g0 + g; // the point's index in the call
    const double *rec = qp.src_hits + (size_t)g * RTMI_HIT_REC;
    const double *L = qp.src_lights + (size_t)l * kLightRec;
    const int kind = (int)L[0];
    const bool sphere = kind == RTMI_PRIM_SPHERE || kind == RTMI_PRIM_UVSPHERE;
    bool ok;
    {
        const double ax = rec[3], ay = rec[4], az = rec[5], bx = rec[6], by = rec[7], bz = rec[8];
        ok = in_range && rec[0] != 0.0 && ::fabs(ax) < big && ::fabs(ay) < big && ::fabs(az) < big // finite: neither inf nor NaN
             && ::fabs(bx) < big && ::fabs(by) < big && ::fabs(bz) < big && dot3(bx, by, bz, bx, by, bz) > 0.0;
    }
    if (qp.src_lambert) {
        const double mf = rec[11];
        const bool known = ok && mf >= 0.0 && mf < (double)qp.src_n_mats;
        ok = known && sc.mat_kind[known ? (int)mf : 0] == RTMI_MAT_LAMBERTIAN;
    }
    Path<double> G; // the sampler's own stream; the ray's (what a ConstantMedium draws from) is load_ray's
    const u64 key = sample_key(qp.src_seed, (u64)gg * (u64)nl + (u64)l, (u64)qp.src_first + (u64)k);
    seed_stream(G, key, 0u);
    double x = 0.0, y = 0.0;
    rand_in_unit_disk_wave<double>(G, ok && sphere, false, x, y);
    // Only the verdict, the disk point and the key cross the cooperative rounds: the record and the light are read again behind them (the fence keeps
    // the compiler from holding thirty doubles in registers through the rounds instead).
    asm volatile("" ::: "memory");
    const double u0 = Real<double>::uniform(mix64(key + RTMI_GOLD)), u1 = Real<double>::uniform(mix64(key + 2ull * RTMI_GOLD)); // draws 0 and 1
    const double px = rec[3], py = rec[4], pz = rec[5];
    double nx = rec[6], ny = rec[7], nz = rec[8];
    const double len2 = dot3(nx, ny, nz, nx, ny, nz);
    const double g0 = L[1], g1 = L[2], g2 = L[3], g3 = L[4], g4 = L[5], area = L[6];
    double time = qp.src_time, wx = 0.0, wy = 0.0, wz = 0.0;
    bool sided = false;
    if (qp.src_view) { const double *v = qp.src_view + (size_t)g * 7; wx = v[3]; wy = v[4]; wz = v[5]; time = v[6]; sided = true; }
    else if (qp.src_view_camera) { double v[7]; pixel_centre_ray(sc, gg, qp.src_nx, qp.src_ny, v); wx = v[3]; wy = v[4]; wz = v[5]; time = v[6]; sided = true; }
    if (sided && dot3(nx, ny, nz, wx, wy, wz) > 0.0) { nx = -nx; ny = -ny; nz = -nz; } // the normal points away from the viewer: the other side
    const double len = ::sqrt(len2);
    nx = nx / len; ny = ny / len; nz = nz / len;
    double qx, qy, qz, sx, sy, sz;
    if (sphere) { // Marsaglia: a uniform point of the unit disk -> a uniform point of the unit sphere
        const double S = x * x + y * y, root = ::sqrt(1.0 - S);
        sx = (2.0 * x) * root; sy = (2.0 * y) * root; sz = 1.0 - 2.0 * S;
        qx = g0 + g3 * sx; qy = g1 + g3 * sy; qz = g2 + g3 * sz;
    } else {
        const double a = g0 + u0 * (g2 - g0), b = g1 + u1 * (g3 - g1);
        sx = kind == RTMI_PRIM_RECT_YZ ? 1.0 : 0.0; sy = kind == RTMI_PRIM_RECT_XZ ? 1.0 : 0.0; sz = kind == RTMI_PRIM_RECT_XY ? 1.0 : 0.0;
        if (kind == RTMI_PRIM_RECT_XY) { qx = a; qy = b; qz = g4; }
        else if (kind == RTMI_PRIM_RECT_XZ) { qx = a; qy = g4; qz = b; }
        else { qx = g4; qy = a; qz = b; }
    }
    const double dx = qx - px, dy = qy - py, dz = qz - pz;
    const double d2 = dot3(dx, dy, dz, dx, dy, dz), cp = dot3(nx, ny, nz, dx, dy, dz), sd = dot3(sx, sy, sz, dx, dy, dz), cl = ::fabs(sd);
    if (sphere) { // the far side of a sphere seen from outside
        const double ex = px - g0, ey = py - g1, ez = pz - g2;
        if (dot3(ex, ey, ez, ex, ey, ez) > g3 * g3 && sd > 0.0) ok = false;
    }
    ok = ok && d2 > 0.0 && cp > 0.0 && cl > 0.0;
    const double w = ((cp * cl) / (d2 * d2)) * area;
    c[0] = ok ? L[7] * w : 0.0; c[1] = ok ? L[8] * w : 0.0; c[2] = ok ? L[9] * w : 0.0;
    q[0] = ok ? px : 0.0; q[1] = ok ? py : 0.0; q[2] = ok ? pz : 0.0;
    q[3] = ok ? dx : 0.0; q[4] = ok ? dy : 0.0; q[5] = ok ? dz : 0.0; q[6] = ok ? time : 0.0;
    return ok;
}

template <typename R, int VARIANT, bool EXT = false, int MSEQ = 0, bool ANY = false, bool COUNT = false, int SRC = SRC_MEMORY>
__global__ void __launch_bounds__(kBlock, EXT ? (MSEQ != 0 ? 3 : RTMI_EXT_MIN_WAVES) : RTMI_MIN_WAVES) query_kernel(ScenePtr scp, QueryParams qp) {
    static_assert(SRC == SRC_MEMORY || (SRC == SRC_PIXEL) != ANY, "the pixel-centre source feeds the closest-hit search, the point sources the any-hit search");
    static_assert(VARIANT >= SCAN_SGPR, "the LDS-staged scans need workgroup barriers: the claim loop is per wave");
    static_assert(!COUNT || (VARIANT == SCAN_BVH && !EXT && sizeof(R) == sizeof(double)), "traversal counters: the FP64 sphere tree only");
    SceneRef sc = *scp;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Prim4<R> *lds = reinterpret_cast<Prim4<R> *>(smem);
    const int lane = threadIdx.x & 63;
    const unsigned total_items = qp.total_items;
    unsigned w_cur = 0, w_end = 0; // this wave's claimed range [w_cur, w_end): wave-uniform
    unsigned n_rays = 0, n_hit = 0; // wave-uniform tallies
    unsigned ntrav[2] = {0u, 0u};
    for (;;) {
        if (w_cur == w_end) {
            unsigned base = 0;
            if (lane == 0) base = atomicAdd(qp.queue, qp.qblock);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base >= total_items) break;
            w_cur = base;
            w_end = min(base + qp.qblock, total_items);
        }
        const unsigned m = w_cur + (unsigned)lane;
        const bool in_range = m < w_end;
        bool active = in_range;
        w_cur = min(w_cur + 64u, w_end);
        const unsigned row = in_range ? m : 0u; // (an idle lane loads row 0 and traces nothing)
        Path<R> P;
        if (SRC == SRC_MEMORY) load_ray<R>(qp.rays + (size_t)row * 7, P);
        else { // a point that yields no ray: an idle lane for this trip, its flag 0
            double q[7];
            if constexpr (SRC == SRC_LIGHT) {
                // the contribution of a ray that reaches its light is written now (no weight is alive across the search), +0.0 where no ray is built
                double c[3];
                active = generate_light_ray(sc, qp, in_range, row, q, c);
                if (in_range && qp.contrib) { double *o = qp.contrib + (size_t)m * 3; o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; }
            } else active = generate_ray<SRC>(sc, qp, in_range, row, q);
            if (in_range && qp.out_rays) {
                double *o = qp.out_rays + (size_t)m * 7;
#pragma unroll
                for (int c = 0; c < 7; ++c) o[c] = q[c];
            }
            load_ray<R>(q, P);
        }
        if (qp.keys) seed_stream(P, qp.keys[row], qp.ctr0);
        R tmin = (R)qp.tmin, tmax = (R)qp.tmax;
        if (qp.t_range) { const double *q = qp.t_range + (size_t)row * 2; tmin = (R)q[0]; tmax = (R)q[1]; }
        R best_t; int best_i;
        intersect_world<R, true, VARIANT, EXT, COUNT, false, MSEQ, false, ANY>(sc, lds, 0, 1, P, active, tmin, tmax, best_t, best_i, COUNT ? ntrav : nullptr);
        const bool hit = active && best_i >= 0;
        const u64 hit_mask = __ballot(hit);
        n_rays += (unsigned)__popcll(__ballot(active));
        n_hit += (unsigned)__popcll(hit_mask);
        if (ANY) {
            if (in_range && qp.occluded) qp.occluded[m] = hit ? 1 : 0;
            if (SRC == SRC_LIGHT && hit && qp.contrib) { // step 7 of the light rule: an occluded ray takes its contribution back
                double *o = qp.contrib + (size_t)m * 3;
                o[0] = 0.0; o[1] = 0.0; o[2] = 0.0;
            }
            if (qp.count) {
                const unsigned g = row / qp.group;
                const unsigned g_prev = (unsigned)__shfl_up((int)g, 1);
                const bool head = active && (lane == 0 || g != g_prev); // the first lane of its group's run in this wave
                const u64 heads = __ballot(head);
                if (head) {
                    const u64 later = lane == 63 ? 0ull : heads >> (lane + 1);
                    const int end = later ? lane + 1 + (__ffsll((long long)later) - 1) : 64; // where the next run begins (idle lanes hold no hit)
                    const u64 run = (end == 64 ? ~0ull : (1ull << end) - 1ull) & ~((1ull << lane) - 1ull);
                    const int k = __popcll(hit_mask & run);
                    if (k) atomicAdd(qp.count + g, k);
                }
            }
        } else if (active) {
            double *o = qp.hits + (size_t)m * RTMI_HIT_REC;
            if (best_i < 0) {
#pragma unroll
                for (int c = 0; c < RTMI_HIT_REC; ++c) o[c] = 0.0;
            } else {
                HitRec<R> h;
                resolve_any<R, EXT>(sc, P, best_t, best_i, h);
                o[0] = 1.0; o[1] = h.orig; o[2] = h.t; o[3] = h.px; o[4] = h.py; o[5] = h.pz;
                o[6] = h.nx; o[7] = h.ny; o[8] = h.nz; o[9] = h.u; o[10] = h.v; o[11] = h.mat;
            }
        }
    }
    if (lane == 0 && n_rays) { atomicAdd(qp.counters, (u64)n_rays); if (n_hit) atomicAdd(qp.counters + 1, (u64)n_hit); }
    if (COUNT) {
        u64 a = ntrav[0], b = ntrav[1];
        for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off); b += __shfl_down(b, off); }
        if (lane == 0) { atomicAdd(qp.trav, a); atomicAdd(qp.trav + 1, b); }
    }
}

// ---- path tracing with next-event estimation on caller-supplied rays (rtmi_render_rays_nee*, rtmi_probe_paths_nee) -------------------------------
// rays_kernel's path -- the same refill, the same closest-hit trip, the same stream -- plus, at every vertex that scattered as a Lambertian, one shadow
// ray towards a sampled point of one uniformly chosen light (THE NEE RULE of rtmi.h).  The light samples draw from keys derived from the path's key and
// the vertex index: the path's own stream is rays_kernel's.  What crosses the any-hit search: the path (as it crosses every closest-hit search) and two
// flags.  The pending contribution T * Le * w * nl waits in the lane's LDS slot, and the running sum `accum` lives there too: neither is a register
// while a tree is walked.
constexpr int kNeeSlots = 6; // doubles per lane in LDS: accum.rgb, pending.rgb; slot s of lane t at nee_lds[s * kBlock + t]
constexpr int kMisSlots = 7; // the MIS instantiations': the lobe value g of the path's last light-sampled vertex behind them
constexpr double kTwoInvPi = 0x1.45f306dc9c883p-1;
struct NeeLights {
    const double *rec; // [n][kLightRec]: set_nee_lights_kernel's copy of the call's light table
    const int *prim;   // [n]: the sampled lights' primitives (what step 6 compares a closing emitter with)
    unsigned n;        // >= 1
};
// The MIS instantiations' light table (set_mis_lights_kernel) carries, behind the kLightRec rows and the primitives, the pick of the MIS rule's step 2:
// rec[kMisRows] = W (+0.0: the uniform pick), then per light {C_l, q_l} from rec[kMisRows + 2].  No other kernel reads past the primitives.
constexpr int kMisRows = RTMI_DIRECT_MAX_LIGHTS * kLightRec + RTMI_DIRECT_MAX_LIGHTS / 2;

// Which of the sampled lights is primitive `orig`: its first index in the list, -1 if none  (at most RTMI_DIRECT_MAX_LIGHTS compares, at a path's end only)
__device__ inline int nee_sampled_light(const NeeLights &nl, int orig) {
    int found = -1;
    for (unsigned l = 0; l < nl.n; ++l) found = found < 0 && nl.prim[l] == orig ? (int)l : found;
    return found;
}

// Steps 2 - 4 of the NEE rule for the vertex j of the path keyed K: the light l, the shadow ray q[7] (zeros where none is built) and the weight w.
// Every lane of the wave calls (the disk sampler is cooperative), the lanes whose vertex takes a light sample with `want`.  As in generate_light_ray
// the rounds stand before the geometry (no operation changes); unlike there the normal is the record's as it is.
// MIS: the light by the MIS rule's step 2, and xmg = {x, m, g} of its steps 4 and 6 for the scattered direction D.
// VOL (THE VOLUME RULE): `iso` lanes sit at an Isotropic scatter -- the record's normal is not read, the lobe is the sphere's 1 / 4 pi.  Both weights and
// both lobe values are formed by every lane and selected: no divergent path.
constexpr double kInv4Pi = 0x1.45f306dc9c883p-4;
// The RIS instantiations' light table (set_ris_lights_kernel) carries, behind the MIS rows (whose q_l are all 1.0), lum_l = (Le.r + Le.g) + Le.b per light.
constexpr int kRisRows = kMisRows + 2 + 2 * RTMI_DIRECT_MAX_LIGHTS;
// What the choice of THE PROPOSAL RULE leaves behind the chosen candidate's ray: S, w^ and r = S / w^ of the chosen one, (Le * m) of it per channel, and
// the number of live candidates.  All zeros where no candidate is live.
struct RisPick { double S, what, r, pend[3]; int live; };
// RIS (THE PROPOSAL RULE; with MIS, without VOL): every listed light proposes a point and a one-pass weighted reservoir keeps one.  The loop index is
// wave-uniform: a light's record is read through the scalar cache, its kind decides one scalar branch for the wave, and in a sphere light's iteration all
// 64 lanes run the disk rounds for the same light.  xmg = {x, m, g} of the chosen candidate; l, w and q are its as well.
template <bool MIS = false, bool VOL = false, bool RIS = false>
__device__ inline bool nee_light_ray(const NeeLights &nl, bool want, u64 K, unsigned j, double px, double py, double pz, double nx, double ny, double nz,
                                     double time, double *q, double &w, int &l, const double *D = nullptr, double *xmg = nullptr, bool iso = false,
                                     RisPick *pick = nullptr) {
    const double big = __builtin_inf();
    const double len2 = dot3(nx, ny, nz, nx, ny, nz);
    bool ok = want && ::fabs(px) < big && ::fabs(py) < big && ::fabs(pz) < big;
    if constexpr (VOL) ok = ok && (iso || (::fabs(nx) < big && ::fabs(ny) < big && ::fabs(nz) < big && len2 > 0.0));
    else ok = ok && ::fabs(nx) < big && ::fabs(ny) < big && ::fabs(nz) < big && len2 > 0.0;
    const bool valid = ok; // (MIS) the vertex itself is sound, whatever becomes of its light sample
    if constexpr (RIS) {
        static_assert(MIS && !VOL, "the proposal rule shares the MIS rule's lobe value and closing weight, and takes no medium");
        const u64 kchoice = sample_key(K, (u64)j, 1ull);
        const double len = ::sqrt(len2);
        nx = nx / len; ny = ny / len; nz = nz / len;
        { // step 6 of the MIS rule, unchanged
            const double a = dot3(nx, ny, nz, D[0], D[1], D[2]), DD = dot3(D[0], D[1], D[2], D[0], D[1], D[2]);
            xmg[2] = valid && a > 0.0 && DD > 0.0 ? ((a * a) * a) / ((DD * DD) * DD) : 0.0;
        }
        double S = 0.0, sel_what = 0.0, sel_w = 0.0, sel_m = 0.0, sel_dx = 0.0, sel_dy = 0.0, sel_dz = 0.0, pend0 = 0.0, pend1 = 0.0, pend2 = 0.0;
        int sel = 0, live = 0;
#pragma nounroll
        for (unsigned k = 0; k < nl.n; ++k) { // nl.n and k are wave-uniform
            typedef const __attribute__((address_space(4))) double *ConstRow;
            ConstRow L = (ConstRow)(unsigned long long)(nl.rec + (size_t)k * kLightRec); // uniform data: scalar loads
            const int kind = __builtin_amdgcn_readfirstlane((int)L[0]);
            const double g0 = L[1], g1 = L[2], g2 = L[3], g3 = L[4], g4 = L[5], area = L[6];
            const double lum = ((ConstRow)(unsigned long long)(nl.rec + kRisRows))[k];
            const u64 key = sample_key(K, (u64)j, 4ull * (u64)k);
            double qx, qy, qz, sx, sy, sz;
            bool far = false;
            if (kind == RTMI_PRIM_SPHERE || kind == RTMI_PRIM_UVSPHERE) { // one branch for the wave: every lane is in the disk rounds
                Path<double> G;
                seed_stream(G, key, 0u);
                double x = 0.0, y = 0.0;
                rand_in_unit_disk_wave<double>(G, valid, false, x, y);
                const double SS = x * x + y * y, root = ::sqrt(1.0 - SS);
                sx = (2.0 * x) * root; sy = (2.0 * y) * root; sz = 1.0 - 2.0 * SS;
                qx = g0 + g3 * sx; qy = g1 + g3 * sy; qz = g2 + g3 * sz;
                const double ex = px - g0, ey = py - g1, ez = pz - g2;
                far = dot3(ex, ey, ez, ex, ey, ez) > g3 * g3; // the far side of a sphere seen from outside, once sd is known
            } else {
                const double u0 = Real<double>::uniform(mix64(key + RTMI_GOLD)), u1 = Real<double>::uniform(mix64(key + 2ull * RTMI_GOLD));
                const double a = g0 + u0 * (g2 - g0), b = g1 + u1 * (g3 - g1);
                sx = kind == RTMI_PRIM_RECT_YZ ? 1.0 : 0.0; sy = kind == RTMI_PRIM_RECT_XZ ? 1.0 : 0.0; sz = kind == RTMI_PRIM_RECT_XY ? 1.0 : 0.0;
                if (kind == RTMI_PRIM_RECT_XY) { qx = a; qy = b; qz = g4; }
                else if (kind == RTMI_PRIM_RECT_XZ) { qx = a; qy = g4; qz = b; }
                else { qx = g4; qy = a; qz = b; }
            }
            const double dx = qx - px, dy = qy - py, dz = qz - pz;
            const double d2 = dot3(dx, dy, dz, dx, dy, dz), cp = dot3(nx, ny, nz, dx, dy, dz), sd = dot3(sx, sy, sz, dx, dy, dz), cl = ::fabs(sd);
            const bool built = valid && !(far && sd > 0.0) && d2 > 0.0 && cp > 0.0 && cl > 0.0;
            const double wk = built ? ((((cp * cp) * (cp * cl)) / ((d2 * d2) * d2)) * area) * kTwoInvPi : 0.0; // x = w: every light proposes, q = 1
            const double mk = wk == big ? 1.0 : wk / (1.0 + wk);
            const double what = lum * mk;
            const bool is_live = built && what > 0.0 && what < big; // (a NaN fails)
            S = is_live ? S + what : S;
            const double u = Real<double>::uniform(mix64(kchoice + RTMI_GOLD * (u64)(k + 1u))); // draw k of the choice's stream
            const bool take = is_live && (live == 0 || u * S < what);
            sel = take ? (int)k : sel;
            sel_what = take ? what : sel_what; sel_w = take ? wk : sel_w; sel_m = take ? mk : sel_m;
            sel_dx = take ? dx : sel_dx; sel_dy = take ? dy : sel_dy; sel_dz = take ? dz : sel_dz;
            pend0 = take ? L[7] * mk : pend0; pend1 = take ? L[8] * mk : pend1; pend2 = take ? L[9] * mk : pend2;
            live += is_live ? 1 : 0;
        }
        ok = live > 0;
        l = sel; w = sel_w;
        xmg[0] = sel_w; xmg[1] = sel_m;
        pick->S = S; pick->what = sel_what; pick->r = ok ? S / sel_what : 0.0; pick->live = live;
        pick->pend[0] = pend0; pick->pend[1] = pend1; pick->pend[2] = pend2;
        q[0] = ok ? px : 0.0; q[1] = ok ? py : 0.0; q[2] = ok ? pz : 0.0;
        q[3] = sel_dx; q[4] = sel_dy; q[5] = sel_dz; q[6] = ok ? time : 0.0;
        return ok;
    }
    const u64 kpick = sample_key(K, (u64)j, 1ull), key = sample_key(K, (u64)j, 0ull);
    const double up = Real<double>::uniform(mix64(kpick + RTMI_GOLD)); // draw 0 of the picking stream
    l = min((int)(up * (double)nl.n), (int)nl.n - 1);
    if constexpr (MIS) {
        const double *M = nl.rec + kMisRows;
        const double W = M[0];
        if (W > 0.0) { // by power: the first light whose running sum exceeds u * W
            const double uw = up * W;
            int pick = (int)nl.n - 1;
            bool found = false;
            for (unsigned k = 0; k < nl.n; ++k) {
                const bool here = !found && uw < M[2 + 2 * k];
                pick = here ? (int)k : pick;
                found = found || here;
            }
            l = pick;
        }
    }
    const double *L = nl.rec + (size_t)l * kLightRec;
    const int kind = (int)L[0];
    const bool sphere = kind == RTMI_PRIM_SPHERE || kind == RTMI_PRIM_UVSPHERE;
    Path<double> G; // the sampler's own stream
    seed_stream(G, key, 0u);
    double x = 0.0, y = 0.0;
    rand_in_unit_disk_wave<double>(G, ok && sphere, false, x, y);
    const double u0 = Real<double>::uniform(mix64(key + RTMI_GOLD)), u1 = Real<double>::uniform(mix64(key + 2ull * RTMI_GOLD)); // draws 0 and 1
    const double g0 = L[1], g1 = L[2], g2 = L[3], g3 = L[4], g4 = L[5], area = L[6];
    const double len = ::sqrt(len2);
    nx = nx / len; ny = ny / len; nz = nz / len;
    if constexpr (MIS) { // step 6: the lobe's value along the scattered ray, less its constant: cos^3 with the direction's length divided out
        const double a = dot3(nx, ny, nz, D[0], D[1], D[2]), DD = dot3(D[0], D[1], D[2], D[0], D[1], D[2]);
        xmg[2] = valid && a > 0.0 && DD > 0.0 ? ((a * a) * a) / ((DD * DD) * DD) : 0.0;
        if constexpr (VOL) { // step 5 of the volume rule: the uniform sphere's density over TWO_INV_PI, with the direction's length divided out
            const double gi = valid && DD > 0.0 ? 0.125 / (DD * ::sqrt(DD)) : 0.0;
            xmg[2] = iso ? gi : xmg[2];
        }
    }
    double qx, qy, qz, sx, sy, sz;
    if (sphere) { // Marsaglia: a uniform point of the unit disk -> a uniform point of the unit sphere
        const double S = x * x + y * y, root = ::sqrt(1.0 - S);
        sx = (2.0 * x) * root; sy = (2.0 * y) * root; sz = 1.0 - 2.0 * S;
        qx = g0 + g3 * sx; qy = g1 + g3 * sy; qz = g2 + g3 * sz;
    } else {
        const double a = g0 + u0 * (g2 - g0), b = g1 + u1 * (g3 - g1);
        sx = kind == RTMI_PRIM_RECT_YZ ? 1.0 : 0.0; sy = kind == RTMI_PRIM_RECT_XZ ? 1.0 : 0.0; sz = kind == RTMI_PRIM_RECT_XY ? 1.0 : 0.0;
        if (kind == RTMI_PRIM_RECT_XY) { qx = a; qy = b; qz = g4; }
        else if (kind == RTMI_PRIM_RECT_XZ) { qx = a; qy = g4; qz = b; }
        else { qx = g4; qy = a; qz = b; }
    }
    const double dx = qx - px, dy = qy - py, dz = qz - pz;
    const double d2 = dot3(dx, dy, dz, dx, dy, dz), cp = dot3(nx, ny, nz, dx, dy, dz), sd = dot3(sx, sy, sz, dx, dy, dz), cl = ::fabs(sd);
    if (sphere) { // the far side of a sphere seen from outside
        const double ex = px - g0, ey = py - g1, ez = pz - g2;
        if (dot3(ex, ey, ez, ex, ey, ez) > g3 * g3 && sd > 0.0) ok = false;
    }
    if constexpr (VOL) ok = ok && d2 > 0.0 && (iso || cp > 0.0) && cl > 0.0;
    else ok = ok && d2 > 0.0 && cp > 0.0 && cl > 0.0;
    w = ok ? ((((cp * cp) * (cp * cl)) / ((d2 * d2) * d2)) * area) * kTwoInvPi : 0.0; // the reference's lobe 2 cos^3 / pi, the light's cosine, the inverse square
    if constexpr (VOL) { // step 3 of the volume rule: the medium scatters uniformly over the sphere
        const double wi = ok ? ((cl / (d2 * ::sqrt(d2))) * area) * kInv4Pi : 0.0;
        w = iso ? wi : w;
    }
    if constexpr (MIS) { // step 4: x = p_scatter / p_light, m = the balance heuristic's share of the light sample
        const double xx = w * nl.rec[kMisRows + 3 + 2 * l];
        xmg[0] = xx;
        xmg[1] = xx == big ? 1.0 : xx / (1.0 + xx);
    }
    q[0] = ok ? px : 0.0; q[1] = ok ? py : 0.0; q[2] = ok ? pz : 0.0;
    q[3] = ok ? dx : 0.0; q[4] = ok ? dy : 0.0; q[5] = ok ? dz : 0.0; q[6] = ok ? time : 0.0;
    return ok;
}

// Steps 2 - 5 of the NEE rule, for the whole wave: `lamb` lanes sit at a vertex that scattered as a Lambertian (P is already the scattered ray: its
// origin is the hit point, its attenuation T).  slot: the lane's LDS column (accum, pending).  rec (probe only, may be null): the vertex' RTMI_NEE_REC row.
// -> the light-sample state of the header: 0 none, 1 built and unoccluded, 2 built and occluded, 3 built no ray.
// MIS (THE MIS RULE): the pending contribution is T * (Le * m), and the lobe value g of the scattered ray goes to the lane's seventh slot, where the path's
// end finds it; rec is then an RTMI_MIS_REC row.
// VOL (THE VOLUME RULE): `lamb` holds the Lambertian and the Isotropic vertices, `iso` the latter; the shadow ray carries a stream of its own, keyed
// sample_key(K, j, 2) at draw 0, from which the media it crosses draw their free-flight distances: the unoccluded flag estimates the transmittance.
// RIS (THE PROPOSAL RULE): the pending contribution is T * ((Le * m) * r) of the chosen candidate; rec is then an RTMI_RIS_REC row.
template <typename R, int VARIANT, bool EXT, bool MIS = false, bool VOL = false, bool RIS = false>
__device__ inline int nee_vertex(SceneRef sc, Prim4<R> *lds, const NeeLights &nl, bool lamb, u64 K, unsigned j, const Path<R> &P, double nx, double ny,
                                 double nz, double *slot, double *rec, bool iso = false) {
    Path<R> S;
    bool ok;
    {
        double q[7], w;
        int l;
        double xmg[3] = {0.0, 0.0, 0.0};
        if constexpr (RIS) {
            const double D[3] = {(double)P.dx, (double)P.dy, (double)P.dz};
            RisPick pk;
            ok = nee_light_ray<true, false, true>(nl, lamb, K, j, (double)P.ox, (double)P.oy, (double)P.oz, nx, ny, nz, (double)P.time, q, w, l, D, xmg, false, &pk);
            if (lamb) slot[6 * kBlock] = xmg[2];
            if (rec && lamb) {
                rec[24] = xmg[0]; rec[25] = xmg[1]; rec[26] = xmg[2];
                rec[28] = pk.S; rec[29] = pk.what; rec[30] = pk.r; rec[31] = (double)pk.live;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double T = (double)(c == 0 ? P.ar : c == 1 ? P.ag : P.ab);
                slot[(3 + c) * kBlock] = ok ? T * (pk.pend[c] * pk.r) : 0.0;
                if (rec && lamb) rec[18 + c] = T;
            }
        } else
        if constexpr (MIS) {
            const double D[3] = {(double)P.dx, (double)P.dy, (double)P.dz};
            ok = nee_light_ray<true, VOL>(nl, lamb, K, j, (double)P.ox, (double)P.oy, (double)P.oz, nx, ny, nz, (double)P.time, q, w, l, D, xmg, iso);
            if (lamb) slot[6 * kBlock] = xmg[2];
            if (rec && lamb) { rec[24] = xmg[0]; rec[25] = xmg[1]; rec[26] = xmg[2]; }
        } else ok = nee_light_ray<false, VOL>(nl, lamb, K, j, (double)P.ox, (double)P.oy, (double)P.oz, nx, ny, nz, (double)P.time, q, w, l, nullptr, nullptr, iso);
        if constexpr (!RIS) {
            const double *L = nl.rec + (size_t)l * kLightRec;
            const double many = (double)nl.n;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double T = (double)(c == 0 ? P.ar : c == 1 ? P.ag : P.ab);
                if constexpr (MIS) slot[(3 + c) * kBlock] = ok ? T * (L[7 + c] * xmg[1]) : 0.0;
                else slot[(3 + c) * kBlock] = ok ? T * ((L[7 + c] * w) * many) : 0.0;
                if (rec && lamb) rec[18 + c] = T;
            }
        }
        if (rec && lamb) { rec[13] = (double)l; rec[14] = q[3]; rec[15] = q[4]; rec[16] = q[5]; rec[17] = w; }
        load_ray<R>(q, S);
        if constexpr (VOL) {
            seed_stream(S, sample_key(K, (u64)j, 2ull), 0u);
            if (rec && lamb) rec[28] = iso ? 1.0 : 0.0;
        }
    }
    R best_t; int best_i;
    intersect_world<R, true, VARIANT, EXT, false, false, 0, false, true>(sc, lds, 0, 1, S, ok, R(0.001), (R)(1.0 - 0.001), best_t, best_i);
    const bool hit = ok && best_i >= 0;
    if (ok && !hit) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double add = slot[(3 + c) * kBlock];
            slot[c * kBlock] = slot[c * kBlock] + add;
            if (rec) rec[21 + c] = add;
        }
    }
    const int state = !lamb ? 0 : !ok ? 3 : hit ? 2 : 1;
    if (rec && lamb) rec[12] = (double)state;
    return state;
}

// Step 7 of the MIS rule: the factor m' on the closing emission of a path that arrives along D at parameter t on sampled light lp, whose record's normal
// is (nx, ny, nz); g = the lobe value its previous vertex left in LDS.  *xq = x', the density ratio at the point the scatter found.
__device__ inline double mis_closing_weight(const NeeLights &nl, int lp, double g, double nx, double ny, double nz, double Dx, double Dy, double Dz, double t,
                                            double *xq) {
    const double len = ::sqrt(dot3(nx, ny, nz, nx, ny, nz));
    nx = nx / len; ny = ny / len; nz = nz / len;
    const double cl = ::fabs(dot3(nx, ny, nz, Dx, Dy, Dz));
    const double x = ((((g * cl) / (t * t)) * nl.rec[(size_t)lp * kLightRec + 6]) * kTwoInvPi) * nl.rec[kMisRows + 3 + 2 * lp];
    *xq = x;
    return x != x ? 0.0 : x == __builtin_inf() ? 1.0 : x / (1.0 + x);
}

struct NeeParams {
    RaysParams rp;   // rays_kernel's arguments; counters: [0] += segments, [2] += shadow rays built, [3] += shadow rays occluded
    NeeLights lights;
};

#ifndef RTMI_NEE_MIN_WAVES
// waves per SIMD rays_nee_kernel is compiled for.  At rays_kernel's 4 (128 VGPRs) the FP64 tree instantiations spill 36 - 68 bytes per lane around the light
// sample; at 3 they take 131 - 141 VGPRs without scratch and measured 4 - 7 % faster (A/B: make variant NAME=nee_w4 FLAGS=-DRTMI_NEE_MIN_WAVES=4)
#define RTMI_NEE_MIN_WAVES 3
#endif
#ifndef RTMI_VOL_MIN_WAVES
// waves per SIMD of the VOL instantiations alone (A/B: make variant NAME=vol_w2 FLAGS=-DRTMI_VOL_MIN_WAVES=2)
#define RTMI_VOL_MIN_WAVES RTMI_NEE_MIN_WAVES
#endif
// MIS (rtmi_render_rays_mis*): THE MIS RULE of rtmi.h -- the same path and the same shadow rays, the balance heuristic on both ends.
// VOL (rtmi_render_rays_vol*, rtmi_render_lit_vol*): THE VOLUME RULE of rtmi.h -- Isotropic vertices sample the lights too, and every shadow ray has a
// stream of its own for the media it crosses.  Mixed-kind FP64 instantiations only: a world of spheres holds no medium.
// RIS (rtmi_render_rays_ris*, rtmi_render_lit_ris*): THE PROPOSAL RULE of rtmi.h -- the MIS rule's path, lobe value and closing weight, with every listed
// light proposing a point at each vertex and one shadow ray towards the candidate a weighted reservoir keeps.
template <typename R, int VARIANT, bool EXT = false, bool MIS = false, int SRC = SRC_MEMORY, bool VOL = false, bool RIS = false>
__global__ void __launch_bounds__(kBlock, VOL ? RTMI_VOL_MIN_WAVES : RTMI_NEE_MIN_WAVES) rays_nee_kernel(ScenePtr scp, NeeParams np) {
    static_assert(SRC == SRC_MEMORY || SRC == SRC_CAMERA || SRC == SRC_CAMERA_TILES, "the path kernels read their rays or build the frame's");
    static_assert(VARIANT >= SCAN_SGPR, "the LDS-staged scans need workgroup barriers: the refill loop is per wave");
    SceneRef sc = *scp;
    __shared__ double nee_lds[(MIS ? kMisSlots : kNeeSlots) * kBlock];
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Prim4<R> *lds = reinterpret_cast<Prim4<R> *>(smem);
    double *slot = nee_lds + threadIdx.x;
    const RaysParams &rp = np.rp;
    const int lane = threadIdx.x & 63;
    const unsigned total_items = rp.total_items;
    unsigned w_cur = 0, w_end = 0; // this wave's claimed range [w_cur, w_end): wave-uniform
    Path<R> P;
    P.ox = P.oy = P.oz = P.dx = P.dy = P.dz = P.time = R(0);
    P.ar = P.ag = P.ab = R(0);
    seed_stream(P, 0ull, 0u); P.depth = 0;
    bool alive = false;
    bool exhausted = (total_items == 0);
    bool sampled = false; // the path's previous vertex took a light sample
    unsigned out_item = 0;
    unsigned nseg = 0, seg = 0, n_built = 0, n_occ = 0; // seg: the path's segment index j
    const R tmin = R(0.001), tmax = Real<R>::tmax();
    for (;;) {
        while (!exhausted) { // every lane of the wave takes part: the loop conditions are wave-uniform
            const u64 dead = __ballot(!alive);
            if (dead == 0) break;
            if (w_cur == w_end) {
                unsigned base = 0;
                if (lane == 0) base = atomicAdd(rp.queue, rp.qblock);
                base = __builtin_amdgcn_readfirstlane(base);
                if (base >= total_items) { exhausted = true; break; }
                w_cur = base;
                w_end = min(base + rp.qblock, total_items);
            }
            const unsigned avail = w_end - w_cur;
            const unsigned rank = (unsigned)__popcll(dead & ((1ull << lane) - 1ull));
            if constexpr (SRC == SRC_CAMERA) {
                const bool has = !alive && rank < avail;
                const unsigned m = w_cur + (has ? rank : 0u); // < total_items
                camera_refill<R>(sc, rp, has, m, P);
                if (has) {
                    out_item = m;
                    alive = true;
                    sampled = false; seg = 0;
                    slot[0] = 0.0; slot[kBlock] = 0.0; slot[2 * kBlock] = 0.0; // accum starts at +0.0
                }
            } else if constexpr (SRC == SRC_CAMERA_TILES) { // a lane whose item holds no pixel stays dead: the next round of this loop deals it another
                const bool has = !alive && rank < avail;
                const unsigned m = w_cur + (has ? rank : 0u); // < total_items
                if (tile_refill<R>(sc, rp, has, m, P)) {
                    out_item = m;
                    alive = true;
                    sampled = false; seg = 0;
                    slot[0] = 0.0; slot[kBlock] = 0.0; slot[2 * kBlock] = 0.0; // accum starts at +0.0
                }
            } else if (!alive && rank < avail) {
                const unsigned m = w_cur + rank; // < total_items
                load_ray<R>(rp.rays + (size_t)m * 7, P);
                u64 key;
                if (rp.keys) key = rp.keys[m];
                else { const unsigned row = rp.row0 + m, g = row / rp.group; key = sample_key(rp.seed, (u64)g, (u64)rp.g_first + (u64)(row - g * rp.group)); }
                seed_stream(P, key, rp.ctr0); P.depth = rp.depth;
                out_item = m;
                alive = true;
                sampled = false; seg = 0;
                slot[0] = 0.0; slot[kBlock] = 0.0; slot[2 * kBlock] = 0.0; // accum starts at +0.0
            }
            w_cur += min((unsigned)__popcll(dead), avail);
        }
        if (!__any(alive ? 1 : 0)) break;
        R best_t; int best_i;
        intersect_world<R, true, VARIANT, EXT, false, false, 0>(sc, lds, 0, 1, P, alive, tmin, tmax, best_t, best_i);
        bool lamb = false, iso = false; // (VOL) lamb: the vertex takes a light sample, Lambertian or Isotropic; iso: the latter
        double nx = 0.0, ny = 0.0, nz = 0.0;
        if (alive) {
            ++nseg;
            R emit[3];
            HitRec<R> h;
            if constexpr (VOL) { alive = shade_segment_vol<R, EXT>(sc, P, best_t, best_i, emit, h, lamb, iso); lamb = lamb || iso; }
            else alive = shade_segment_nee<R, EXT>(sc, P, best_t, best_i, emit, h, lamb);
            nx = (double)h.nx; ny = (double)h.ny; nz = (double)h.nz;
            if (!alive) { // step 6: a sampled light's emission was already counted at the previous vertex
                double *out = rp.samples + (size_t)out_item * 3;
                if constexpr (MIS) { // step 7 of the MIS rule: that emission is weighted, not dropped -- the scatter's share of the two strategies
                    const int lp = sampled && best_i >= 0 ? nee_sampled_light(np.lights, best_i) : -1;
                    double mw = 1.0, xq;
                    if (lp >= 0) mw = mis_closing_weight(np.lights, lp, slot[6 * kBlock], nx, ny, nz, (double)P.dx, (double)P.dy, (double)P.dz, (double)h.t, &xq);
#pragma unroll
                    for (int c = 0; c < 3; ++c) out[c] = slot[c * kBlock] + (double)emit[c] * mw;
                } else {
                    const bool drop = sampled && best_i >= 0 && nee_sampled_light(np.lights, best_i) >= 0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) out[c] = slot[c * kBlock] + (drop ? 0.0 : (double)emit[c]);
                }
            }
        }
        if (__any(lamb ? 1 : 0)) { // wave-uniform: all 64 lanes enter the disk rounds and the any-hit search
            const int state = nee_vertex<R, VARIANT, EXT, MIS, VOL, RIS>(sc, lds, np.lights, lamb, P.key, seg, P, nx, ny, nz, slot, nullptr, iso);
            n_built += state == 1 || state == 2 ? 1u : 0u;
            n_occ += state == 2 ? 1u : 0u;
        }
        sampled = lamb;
        ++seg;
    }
    // segments and shadow rays: wave reductions, one atomic per wave and counter
    unsigned n = nseg, b = n_built, o = n_occ;
    for (int off = 32; off > 0; off >>= 1) { n += __shfl_down(n, off); b += __shfl_down(b, off); o += __shfl_down(o, off); }
    if (lane == 0) {
        if (n) atomicAdd(rp.counters, (u64)n);
        if (b) atomicAdd(rp.counters + 2, (u64)b);
        if (o) atomicAdd(rp.counters + 3, (u64)o);
    }
}

// rtmi_probe_paths_nee: one path per thread through the same device functions, each vertex logged as RTMI_NEE_REC doubles
struct NeeProbeParams {
    int n;
    const double *rays;
    const u64 *keys;
    unsigned ctr0;
    int depth;
    double *out_rgb;   // [n][3]
    u64 *out_nseg;     // [n], or null
    void *out_end;     // [n], or null: int32, 1 where the closing emission was dropped; MIS: doubles, the factor on the closing emission
    double *log;       // [n][max_seg][RTMI_NEE_REC] (MIS: RTMI_MIS_REC), zeroed before the launch, or null
    int max_seg;
    int *out_nlog;     // [n], or null
    NeeLights lights;  // n == 0: no vertex takes a light sample
};

// VOL (rtmi_probe_paths_vol): the rows are RTMI_VOL_REC doubles and out_end is the factor on the closing emission under either rule (the NEE rule's
// 0.0 where it is dropped)
// RIS (rtmi_probe_paths_ris): the rows are RTMI_RIS_REC doubles
template <typename R, int VARIANT, bool EXT = false, bool MIS = false, bool VOL = false, bool RIS = false>
__global__ void __launch_bounds__(kBlock) probe_paths_nee_kernel(ScenePtr scp, NeeProbeParams pp) {
    static_assert(VARIANT >= SCAN_SGPR, "the loop is per wave, as rays_nee_kernel's");
    SceneRef sc = *scp;
    __shared__ double nee_lds[(MIS ? kMisSlots : kNeeSlots) * kBlock];
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Prim4<R> *lds = reinterpret_cast<Prim4<R> *>(smem);
    double *slot = nee_lds + threadIdx.x;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    bool alive = k < pp.n;
    const size_t row = (size_t)(alive ? k : 0);
    Path<R> P;
    load_ray<R>(pp.rays + row * 7, P);
    seed_stream(P, alive ? pp.keys[k] : 0ull, pp.ctr0); P.depth = pp.depth;
    constexpr int kRec = RIS ? RTMI_RIS_REC : VOL ? RTMI_VOL_REC : MIS ? RTMI_MIS_REC : RTMI_NEE_REC;
    double *log = pp.log ? pp.log + row * (size_t)pp.max_seg * kRec : nullptr;
    int nlog = 0, dropped = 0;
    double weight = 1.0; // (MIS) the factor on the closing emission
    u64 nseg = 0;
    unsigned seg = 0;
    bool sampled = false;
    const R tmin = R(0.001), tmax = Real<R>::tmax();
    double rgb[3] = {0.0, 0.0, 0.0};
    slot[0] = 0.0; slot[kBlock] = 0.0; slot[2 * kBlock] = 0.0;
    while (__any(alive ? 1 : 0)) {
        R best_t; int best_i;
        intersect_world<R, true, VARIANT, EXT, false, false, 0>(sc, lds, 0, 1, P, alive, tmin, tmax, best_t, best_i);
        bool lamb = false, iso = false;
        double nx = 0.0, ny = 0.0, nz = 0.0;
        double *rec = nullptr;
        if (alive) {
            ++nseg;
            R emit[3];
            HitRec<R> h;
            if constexpr (VOL) { alive = shade_segment_vol<R, EXT>(sc, P, best_t, best_i, emit, h, lamb, iso); lamb = lamb || iso; }
            else alive = shade_segment_nee<R, EXT>(sc, P, best_t, best_i, emit, h, lamb);
            lamb = lamb && pp.lights.n > 0;
            nx = (double)h.nx; ny = (double)h.ny; nz = (double)h.nz;
            if (log && best_i >= 0 && nlog < pp.max_seg) { // shade_segment's record (a miss logs none); [12..23] stay zeros unless the vertex takes a light sample
                rec = log + (size_t)nlog * kRec;
                rec[0] = h.orig; rec[1] = h.t; rec[2] = h.px; rec[3] = h.py; rec[4] = h.pz; rec[5] = h.nx; rec[6] = h.ny; rec[7] = h.nz;
                rec[8] = alive ? P.dx : 0; rec[9] = alive ? P.dy : 0; rec[10] = alive ? P.dz : 0; rec[11] = alive ? 1.0 : 0.0;
                ++nlog;
            }
            if (!alive) {
                if constexpr (MIS) {
                    const int lp = sampled && best_i >= 0 ? nee_sampled_light(pp.lights, best_i) : -1;
                    if (lp >= 0) {
                        double xq;
                        weight = mis_closing_weight(pp.lights, lp, slot[6 * kBlock], nx, ny, nz, (double)P.dx, (double)P.dy, (double)P.dz, (double)h.t, &xq);
                        if (rec) rec[27] = xq;
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) rgb[c] = slot[c * kBlock] + (double)emit[c] * weight;
                } else {
                    const bool drop = sampled && best_i >= 0 && nee_sampled_light(pp.lights, best_i) >= 0;
                    dropped = drop ? 1 : 0;
                    if constexpr (VOL) weight = drop ? 0.0 : 1.0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) rgb[c] = slot[c * kBlock] + (drop ? 0.0 : (double)emit[c]);
                }
            }
        }
        if (__any(lamb ? 1 : 0)) nee_vertex<R, VARIANT, EXT, MIS, VOL, RIS>(sc, lds, pp.lights, lamb, P.key, seg, P, nx, ny, nz, slot, rec, iso);
        sampled = lamb;
        ++seg;
    }
    if (k < pp.n) {
        pp.out_rgb[3 * k] = rgb[0]; pp.out_rgb[3 * k + 1] = rgb[1]; pp.out_rgb[3 * k + 2] = rgb[2];
        if (pp.out_nseg) pp.out_nseg[k] = nseg;
        if (pp.out_end) {
            if constexpr (MIS || VOL) static_cast<double *>(pp.out_end)[k] = weight;
            else static_cast<int *>(pp.out_end)[k] = dropped;
        }
        if (pp.out_nlog) pp.out_nlog[k] = nlog;
    }
}

// ---- edge-aware denoiser (rtmi_denoise*): an a-trous wavelet filter over planar FP64 images -----------------------------------------------------
// Planes of nx * ny doubles: colour r, g, b and the variance of the mean V (two sets: a pass reads one and writes the other), then normal xyz,
// albedo rgb and depth (read only).  Lanes run along x: every tap of a wave is one contiguous run per plane.
constexpr int kDnState = 4, kDnFeat = 7;
constexpr double kDnTiny = 0x1p-200; // E of rtmi.h

// interleaved inputs -> planes.  V = se * se (0 without stderr_in)
__global__ void __launch_bounds__(kBlock) denoise_load_kernel(const double *__restrict__ lin, const double *__restrict__ se, const double *__restrict__ feat,
                                                              size_t n, double *__restrict__ state, double *__restrict__ fplanes) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    state[p] = lin[3 * p]; state[n + p] = lin[3 * p + 1]; state[2 * n + p] = lin[3 * p + 2];
    double v = 0.0;
    if (se) { const double e = se[p]; v = e * e; }
    state[3 * n + p] = v;
    if (feat) {
        const double *f = feat + 8 * p;
        fplanes[p] = f[3]; fplanes[n + p] = f[4]; fplanes[2 * n + p] = f[5];
        fplanes[3 * n + p] = f[0]; fplanes[4 * n + p] = f[1]; fplanes[5 * n + p] = f[2];
        fplanes[6 * n + p] = f[6];
    }
}

// One pass with tap distance `step`.  use_c / use_n / use_a / use_d are launch-uniform: a term that is off is not evaluated.  s*2 = sigma squared.
__global__ void __launch_bounds__(kBlock) denoise_pass_kernel(const double *__restrict__ in, double *__restrict__ out, const double *__restrict__ fp,
                                                              int nx, int ny, int step, int use_c, int use_n, int use_a, int use_d,
                                                              double sc2, double sn2, double sa2, double sd2) {
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u)), y = (int)(blockIdx.y * (kBlock / 64) + (threadIdx.x >> 6));
    if (x >= nx || y >= ny) return;
    const size_t n = (size_t)nx * (size_t)ny, p = (size_t)y * (size_t)nx + (size_t)x;
    const double c0 = in[p], c1 = in[n + p], c2 = in[2 * n + p], vp = in[3 * n + p];
    const double big = __builtin_inf();
    const bool centre_ok = ::fabs(c0) < big && ::fabs(c1) < big && ::fabs(c2) < big; // finite: neither inf nor NaN
    double n0 = 0, n1 = 0, n2 = 0, a0 = 0, a1 = 0, a2 = 0, dp = 0;
    if (use_n) { n0 = fp[p]; n1 = fp[n + p]; n2 = fp[2 * n + p]; }
    if (use_a) { a0 = fp[3 * n + p]; a1 = fp[4 * n + p]; a2 = fp[5 * n + p]; }
    if (use_d) dp = fp[6 * n + p];
    double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, sv = 0.0;
    if (centre_ok) {
        for (int dy = -2; dy <= 2; ++dy) {
            const int qy = y + dy * step;
            if (qy < 0 || qy >= ny) continue; // (wave-uniform)
            const double hy = dy == 0 ? 0.375 : ((dy == 1 || dy == -1) ? 0.25 : 0.0625);
            for (int dx = -2; dx <= 2; ++dx) {
                const int qx = x + dx * step;
                if (qx < 0 || qx >= nx) continue;
                const double hx = dx == 0 ? 0.375 : ((dx == 1 || dx == -1) ? 0.25 : 0.0625);
                const size_t q = (size_t)qy * (size_t)nx + (size_t)qx;
                const double q0 = in[q], q1 = in[n + q], q2 = in[2 * n + q], vq = in[3 * n + q];
                if (!(::fabs(q0) < big && ::fabs(q1) < big && ::fabs(q2) < big)) continue;
                double xx = 0.0;
                if (use_c) {
                    const double e0 = c0 - q0, e1 = c1 - q1, e2 = c2 - q2;
                    xx = xx + ((e0 * e0 + e1 * e1) + e2 * e2) / (sc2 * (vp + vq) + kDnTiny);
                }
                if (use_n) {
                    const double e0 = n0 - fp[q], e1 = n1 - fp[n + q], e2 = n2 - fp[2 * n + q];
                    xx = xx + ((e0 * e0 + e1 * e1) + e2 * e2) / sn2;
                }
                if (use_a) {
                    const double e0 = a0 - fp[3 * n + q], e1 = a1 - fp[4 * n + q], e2 = a2 - fp[5 * n + q];
                    xx = xx + ((e0 * e0 + e1 * e1) + e2 * e2) / sa2;
                }
                if (use_d) {
                    const double dq = fp[6 * n + q], e = dp - dq, pp = dp * dp, qq = dq * dq;
                    xx = xx + (e * e) / (sd2 * (qq > pp ? qq : pp) + kDnTiny);
                }
                if (xx != xx) continue;
                const double r = 1.0 / (1.0 + xx);
                const double w = (hy * hx) * ((r * r) * (r * r));
                if (!(w > 0.0)) continue; // 0 (x = +inf) or NaN
                sw = sw + w;
                s0 = s0 + w * q0; s1 = s1 + w * q1; s2 = s2 + w * q2;
                sv = sv + (w * w) * vq;
            }
        }
    }
    if (sw != 0.0) { // (never with a non-finite centre)
        out[p] = s0 / sw; out[n + p] = s1 / sw; out[2 * n + p] = s2 / sw; out[3 * n + p] = sv / (sw * sw);
    } else { out[p] = c0; out[n + p] = c1; out[2 * n + p] = c2; out[3 * n + p] = vp; }
}

// planes -> interleaved outputs.  se_copy != null: out_stderr copies it (iterations = 0); else sqrt(V) (V = 0 without stderr_in)
__global__ void __launch_bounds__(kBlock) denoise_store_kernel(const double *__restrict__ state, size_t n, const double *__restrict__ se_copy,
                                                               double *__restrict__ out_linear, unsigned char *__restrict__ out_rgb8,
                                                               double *__restrict__ out_stderr) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    for (int c = 0; c < 3; ++c) {
        const double m = state[(size_t)c * n + p];
        if (out_linear) out_linear[3 * p + c] = m;
        if (out_rgb8) out_rgb8[3 * p + c] = quantise8(m);
    }
    if (out_stderr) out_stderr[p] = se_copy ? se_copy[p] : ::sqrt(state[3 * n + p]);
}

// ---- temporal accumulation (rtmi_reproject*): the previous frame gathered through both cameras and blended with the current one -----------------------
// One thread per pixel, lanes along x (denoise_pass_kernel's launch shape).  It reads the interleaved buffers as the callers hold them and writes every
// output, the 8-bit frame included: one launch per call.  The cameras and the constants the host computes from the previous one are kernel arguments.
struct ReprojectParams {
    int nx, ny;
    int use_d, use_n, use_a;              // launch-uniform: a test that is off is not evaluated and its values are not loaded
    double co[3], cl[3], ch[3], cv[3];    // current camera: origin, lleft, horiz, vert
    double po[3], ph[3], pv[3];           // previous camera: origin, horiz, vert
    double a[3], n[3], nn, A;             // a = l' - o', n = h' x v', nn = n . n, A = a . n (rtmi.h)
    double cur_weight, max_history, sd2, sn2, sa2; // s*2 = sigma squared
    const double *prev_lin, *prev_w, *prev_se, *prev_feat;
    const double *cur_lin, *cur_se, *cur_feat;    // (no __restrict__: the outputs may alias the current frame's buffers)
    double *out_lin; unsigned char *out_q; double *out_w, *out_se;
    u64 *counters;                        // [0] = pixels, [1] += pixels that took history; may be null
};

__global__ void __launch_bounds__(kBlock) reproject_kernel(ReprojectParams rp) {
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u)), y = (int)(blockIdx.y * (kBlock / 64) + (threadIdx.x >> 6));
    const bool inside = x < rp.nx && y < rp.ny;
    bool took = false;
    if (inside) {
        const double big = __builtin_inf();
        const size_t p = (size_t)y * (size_t)rp.nx + (size_t)x;
        const double c0 = rp.cur_lin[3 * p], c1 = rp.cur_lin[3 * p + 1], c2 = rp.cur_lin[3 * p + 2];
        const double se_c = rp.cur_se ? rp.cur_se[p] : 0.0;
        const double *f = rp.cur_feat + 8 * p;
        const double depth = f[6];
        double n0 = 0, n1 = 0, n2 = 0, a0 = 0, a1 = 0, a2 = 0;
        if (rp.use_n) { n0 = f[3]; n1 = f[4]; n2 = f[5]; }
        if (rp.use_a) { a0 = f[0]; a1 = f[1]; a2 = f[2]; }
        bool ok = f[7] == 1.0 && ::fabs(c0) < big && ::fabs(c1) < big && ::fabs(c2) < big;
        // the world point and its place in the previous frame: every lane computes (a pixel that is not `ok` computes on whatever it holds and
        // its result is not used), so that the loads of the four taps below do not wait behind a chain of branches
        const double u = ((double)x + 0.5) / (double)rp.nx, v = ((double)(rp.ny - 1 - y) + 0.5) / (double)rp.ny;
        const double d0 = ((rp.cl[0] + u * rp.ch[0]) + v * rp.cv[0]) - rp.co[0];
        const double d1 = ((rp.cl[1] + u * rp.ch[1]) + v * rp.cv[1]) - rp.co[1];
        const double d2 = ((rp.cl[2] + u * rp.ch[2]) + v * rp.cv[2]) - rp.co[2];
        const double len = ::sqrt((d0 * d0 + d1 * d1) + d2 * d2);
        const double s = depth / len;
        const double q0 = (rp.co[0] + s * d0) - rp.po[0], q1 = (rp.co[1] + s * d1) - rp.po[1], q2 = (rp.co[2] + s * d2) - rp.po[2];
        const double t = rp.A / ((q0 * rp.n[0] + q1 * rp.n[1]) + q2 * rp.n[2]);
        ok = ok && t > 0.0;
        const double X0 = t * q0 - rp.a[0], X1 = t * q1 - rp.a[1], X2 = t * q2 - rp.a[2];
        const double up = (((X1 * rp.pv[2] - X2 * rp.pv[1]) * rp.n[0] + (X2 * rp.pv[0] - X0 * rp.pv[2]) * rp.n[1]) +
                           (X0 * rp.pv[1] - X1 * rp.pv[0]) * rp.n[2]) / rp.nn;
        const double vp = (((rp.ph[1] * X2 - rp.ph[2] * X1) * rp.n[0] + (rp.ph[2] * X0 - rp.ph[0] * X2) * rp.n[1]) +
                           (rp.ph[0] * X1 - rp.ph[1] * X0) * rp.n[2]) / rp.nn;
        double fx = up * (double)rp.nx - 0.5, fy = (double)(rp.ny - 1) - (vp * (double)rp.ny - 0.5);
        ok = ok && fx > -1.0 && fx < (double)rp.nx && fy > -1.0 && fy < (double)rp.ny; // (a NaN fails)
        if (!ok) { fx = 0.0; fy = 0.0; }                                               // (the conversions below are in range)
        const double dist = ::sqrt((q0 * q0 + q1 * q1) + q2 * q2);
        const double flx = ::floor(fx), fly = ::floor(fy), ax = fx - flx, ay = fy - fly;
        const int x0 = (int)flx, y0 = (int)fly;
        double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, sn = 0.0, st = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int tx = k & 1, ty = k >> 1, gx = x0 + tx, gy = y0 + ty;
            bool acc = ok && gx >= 0 && gx < rp.nx && gy >= 0 && gy < rp.ny;
            // a tap outside the image reads the nearest pixel inside (and is not accepted): every address below is in bounds for every lane
            const int cx = gx < 0 ? 0 : (gx >= rp.nx ? rp.nx - 1 : gx), cy = gy < 0 ? 0 : (gy >= rp.ny ? rp.ny - 1 : gy);
            const size_t g = (size_t)cy * (size_t)rp.nx + (size_t)cx;
            const double *fq = rp.prev_feat + 8 * g;
            const double covq = fq[7], wq = rp.prev_w[g];
            const double p0 = rp.prev_lin[3 * g], p1 = rp.prev_lin[3 * g + 1], p2 = rp.prev_lin[3 * g + 2];
            const double b = (tx ? ax : 1.0 - ax) * (ty ? ay : 1.0 - ay);
            acc = acc && b > 0.0 && covq == 1.0 && wq > 0.0 && wq < big && ::fabs(p0) < big && ::fabs(p1) < big && ::fabs(p2) < big;
            double seq = 0.0;
            if (rp.prev_se) { seq = rp.prev_se[g]; acc = acc && seq == seq; }
            if (rp.use_d) {
                const double dq = fq[6], e = dq - dist, m = dq > dist ? dq : dist;
                acc = acc && e * e <= rp.sd2 * (m * m);
            }
            if (rp.use_n) {
                const double e0 = n0 - fq[3], e1 = n1 - fq[4], e2 = n2 - fq[5];
                acc = acc && (e0 * e0 + e1 * e1) + e2 * e2 <= rp.sn2;
            }
            if (rp.use_a) {
                const double e0 = a0 - fq[0], e1 = a1 - fq[1], e2 = a2 - fq[2];
                acc = acc && (e0 * e0 + e1 * e1) + e2 * e2 <= rp.sa2;
            }
            if (acc) {
                sw = sw + b;
                s0 = s0 + b * p0; s1 = s1 + b * p1; s2 = s2 + b * p2;
                sn = sn + b * wq;
                st = st + b * (seq * seq);
            }
        }
        double o0 = c0, o1 = c1, o2 = c2, ow = rp.cur_weight, ose = se_c;
        if (sw != 0.0) {
            took = true;
            double nh = sn / sw;
            if (nh > rp.max_history) nh = rp.max_history;
            const double w = nh + rp.cur_weight, cw = rp.cur_weight;
            o0 = (nh * (s0 / sw) + cw * c0) / w; o1 = (nh * (s1 / sw) + cw * c1) / w; o2 = (nh * (s2 / sw) + cw * c2) / w;
            ow = w;
            if (rp.out_se) ose = ::sqrt(((nh * nh) * (st / sw) + (cw * cw) * (se_c * se_c)) / (w * w));
        }
        if (rp.out_lin) { rp.out_lin[3 * p] = o0; rp.out_lin[3 * p + 1] = o1; rp.out_lin[3 * p + 2] = o2; }
        if (rp.out_q) { rp.out_q[3 * p] = quantise8(o0); rp.out_q[3 * p + 1] = quantise8(o1); rp.out_q[3 * p + 2] = quantise8(o2); }
        if (rp.out_w) rp.out_w[p] = ow;
        if (rp.out_se) rp.out_se[p] = ose;
    }
    // The counters.  Every pixel of the frame is visited, so the first is nx * ny: one lane stores it.  The second takes one atomic per wave that
    // found history.  (Two atomics per wave, as feature_kernel counts, were 0.67 ms of a 0.82 ms call at 1920 x 1080: 32 400 waves adding to one
    // cache line wait for each other, and this kernel is too short to hide it.  DESIGN.md section 7h.)
    if (rp.counters) {
        const u64 hist = __ballot(took);
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) rp.counters[0] = (u64)rp.nx * (u64)rp.ny;
        if ((threadIdx.x & 63u) == 0 && hist) atomicAdd(rp.counters + 1, (u64)__popcll(hist));
    }
}

// What a progressive frame was started with: a continuation must match it field for field
struct ProgKey {
    uint64_t scene_serial = 0, scene_revision = 0, seed = 0;
    int nx = 0, ny = 0, depth = 0, precision = 0;
    int rg[4] = {0, 0, 0, 0};
    int first = 0, stride = 1; // the dealing: the frame's local tiles are the global tiles first, first + stride, ... ((0, 1): every tile of the region)
};

// A context's progressive frame (rtmi_render_progressive*): the state frame_fold_kernel keeps (sums in the precision of the frame, Welford
// mean / M2 in double), the cumulative metrics counters, and the key; k = samples [0, k) it holds (0 = no frame).  Its own buffers: a one-shot
// render on the same context in between does not touch it.
// Per-tile state (rtmi_render_adaptive*): n_tiles local tiles of valid_pixels pixels inside the image and the region.  While `adaptive` is false every
// tile is active with n_t = k and the arrays below are not in use (rtmi_render_progressive* never reads them); the first adaptive call fills them.
// The active list is its own pair of arrays (c->tile_ids is rewritten by any other render on the context), double-buffered: the compaction reads
// list `cur` and writes the other.  n_active, active_pixels and pixel_samples mirror the device's state on the host.
struct ProgFrame {
    DevBuf sums, mean, m2, counters;
    DevBuf act_tiles[2], act_slots[2], n_t, keep, meta;
    ProgKey key;
    int k = 0;
    bool adaptive = false;
    int cur = 0, n_tiles = 0, n_active = 0;
    long long valid_pixels = 0, active_pixels = 0, pixel_samples = 0;
    int *meta_host = nullptr;  // pinned copy of `meta`: a dealt call's copy-back must not block the host while the other replicas are launched
    bool meta_pending = false; // a dealt call traced tiles: meta_host holds the next active list's length once its stream is synchronised
    void release() {
        sums.release(); mean.release(); m2.release(); counters.release();
        for (int i = 0; i < 2; ++i) { act_tiles[i].release(); act_slots[i].release(); }
        n_t.release(); keep.release(); meta.release();
        if (meta_host) (void)hipHostFree(meta_host);
        meta_host = nullptr; meta_pending = false;
        k = 0; adaptive = false; cur = n_tiles = n_active = 0; valid_pixels = active_pixels = pixel_samples = 0;
    }
};

// what an adaptive call adds to the sample passes of a progressive one
struct AdaptiveCall {
    double eps = 0.0;
    int k_before = 0; // the frame's k when the call started
};

} // namespace

struct rtmi_ctx {
    uint32_t magic = 0x52544d49u;
    int device = 0;
    uint32_t flags = 0;
    hipStream_t stream = nullptr;
    int cus = 0;
    int lds_per_cu = 0;
    size_t hbm = 0;
    std::string arch;
    int blocks_per_cu = 8; // workgroups per CU in the persistent grid (4 resident; the rest start as others drain: shorter tail)
    int64_t workspace_bytes = (int64_t)64 << 30; // sample-buffer budget (HBM is 288 GB; allocated as needed): 1920x1080x256 (12.7 GB of samples) renders in one pass, 3840x2160x512 in two
    int accel = RTMI_ACCEL_BVH; // bit-identical to the flat Hitlist scan and what every reference scene builds (scene.clj:332: make-bvh)
    int scan_variant = SCAN_SGPR_CULL;
    int max_lds_bytes = 64 * 1024 - 64; // static-sphere LDS tile budget per workgroup
    // workspace
    DevBuf samples, accum, tiles, tile_ids, counters;
    DevBuf io;    // every host form's staging (HostIo): idle between calls, each of which ends with the stream synchronised
    DevBuf multi; // rtmi_render_multi*: this replica's record (tiles + counters); on replica 0 the gathered records of all replicas
    hipEvent_t ev_done = nullptr, ev_g0 = nullptr, ev_g1 = nullptr; // multi-device: render finished / gather interval on replica 0
    bool have_gather = false;
    int last_gather_path = RTMI_GATHER_NONE; // how the last rtmi_render_multi* on this context (as replica 0) gathered
    // copy-branch gather: replica 0's stream copies OUT of this replica's record; the event (created on replica 0's device, recorded on
    // its stream after the copy) is what this replica's stream waits for before it renders into the record again
    hipEvent_t ev_consumed = nullptr;
    int ev_consumed_device = -1;
    bool consume_pending = false;
    int defer_emitters = 1;    // option "defer_emitters": a scene's deferred emitter (DevScene::defer_mat) is finished by the fold; 0: every render stores 3-real samples
    int fail_next_render = 0;  // option "test_fail_next_render" (test hook): the next render on this context fails before it launches anything
    int fail_allocs = 0;       // option "test_fail_allocs" (test hook): the next n sample-buffer allocations fail as if HBM were exhausted
    int last_accel = -1;       // RTMI_ACCEL_* the most recent render ran (rtmi_last_accel): option "flat_below" can answer a request for the tree with the scan
    int last_passes = 0;       // sample passes of the most recent render (rtmi_last_passes)
    int last_record_reals = 0; // reals per sample record of the most recent render that traced (rtmi_last_record_reals): 4 = it deferred, 3 = it did not
    int last_grid = 0; // workgroups of the last trace launch (diagnostics)
    std::map<std::pair<const void *, size_t>, int> occupancy; // resident workgroups per CU by (kernel, dynamic LDS bytes)
    std::vector<int> tile_ids_host;
    int tile_key[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    std::vector<hipEvent_t> events_r; // RTMI_FLAG_TIMING: after the reduction that follows launch k
    double last_reduce_ms = 0.0;      // of the window rtmi_last_trace_ms closed last
    int last_reduce_launches = 0;
    int count_traversal = 0;      // option "count_traversal": run the COUNT instantiation of the BVH kernels
    int flat_below = 24;          // option "flat_below": mixed-kind scenes with fewer primitives answer accel = BVH with the flat scan (same image; 3 - 10 % faster there)
    bool suspend_lanes_set = false; // the option was set by the host (else mixed-kind trees take their own default, see the launch)
    int suspend_lanes = 8;        // option "suspend_lanes": threshold of the time-sliced BVH traversal (0 = plain while-while loop); 6 .. 12 within 0.4 % (C3 69.3 / 69.2 / 69.5 ms at 6 / 10 / 12; 18: 70.7, 24: 73.6)
    hipStream_t last_stream = nullptr; // stream of the most recent render (rtmi_last_traversal_counters synchronises on it)
    long long tile_valid_pixels = 0;
    ProgFrame prog; // at most one progressive frame per context
    DevBuf feat_cnt;  // rtmi_render_features_device: the counters nobody asked for
    DevBuf dn_planes; // rtmi_denoise*: the filter's planes (two colour + variance sets, the feature planes)
    DevBuf rays_ws;   // rtmi_render_rays*: the per-ray radiance nobody asked for (one pass of it)
    DevBuf occ_ws;    // rtmi_ambient_occlusion*: the first-hit records and the per-pixel counts nobody asked for
    DevBuf nee_ws;    // rtmi_render_rays_nee*, rtmi_probe_paths_nee: the light table and the sampled lights' primitives
    DevBuf retire_ws; // rtmi_tiles_retire*: the keep flags, the surviving tiles and their slots, the two ints of the compaction's meta
    DevBuf direct_ws; // rtmi_direct_irradiance*, rtmi_render_direct*: the light table, then the records and irradiance nobody asked for, then one pass of contributions
    // timing
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    int events_used = 0;
};

struct rtmi_scene {
    uint32_t magic = 0x52545343u;
    rtmi_ctx *ctx = nullptr;
    DevScene dev{};             // host copy of the descriptor
    ScenePtr d_dev = nullptr;   // the descriptor in HBM (what the kernels read)
    std::vector<void *> allocs;       // the descriptor and what rtmi_scene_set_perlin / _images uploaded
    std::vector<void *> table_allocs; // the tables pack_scene built (records, trees, cull entries): what a camera whose shutter does not fit replaces
    size_t table_bytes = 0;           // bytes of table_allocs (part of device_bytes)
    size_t device_bytes = 0;  // HBM the scene occupies = what its creation uploads (rtmi_scene_device_bytes)
    int n_prims = 0, n_mats = 0, n_tex = 0;
    int bvh_node_count = 0;   // inner nodes of the device's tree
    int bvh_depth = 0;        // deepest leaf of the device's tree(s)
    bool uses_perlin = false; // a Perlin texture is present: rtmi_scene_set_perlin must have been called before rendering
    int max_image = -1;       // highest ImageMap index: rtmi_scene_set_images must cover it
    bool have_perlin = false;
    uint64_t serial = 0;      // creation serial (a scene created at a destroyed scene's address is still another scene: progressive frame key)
    uint64_t revision = 0;    // incremented by every rtmi_scene_set_* call that changes the scene
    std::vector<int> host_kind; // primitive kinds (boundary flag removed), for argument checks
    bool has_moving = false;    // a RTMI_PRIM_MOVING primitive is present: the trees and cull entries hold for the shutter interval [dev.cull_t_lo, dev.cull_t_hi] only
    std::map<int, std::array<double, 5>> media_fast_of; // medium primitive -> {density, c.xyz, r*r} when it and its boundary are one plain sphere without wrappers (DevScene::media_fast)
    PackedMaterials mat;   // host copy of the eleven material tables as they lie in HBM: what rtmi_scene_set_materials_stream compares an edit with, row by row
    bool geom_ext = false; // the geometry's share of dev.has_ext (PackedScene::geom_ext): an edit of the materials fits if it leaves dev.has_ext as it is
    TreeBuild tree;        // what the trees in HBM were built with: rtmi_scene_set_geometry judges every edit against it
    // rtmi_scene_set_geometry: made by the first edit after a build, dropped by every rebuild (whoever asked for it)
    struct GeoEdit {
        bool ready = false;
        PackedScene tab;             // host copy of the geometry tables as they lie in HBM (P.d, P.M and the trees are not used)
        GeomExtras X;                // ... and the world boxes they were packed with
        std::vector<char> displaced; // per world primitive: it left its place in the trees and joined the big list
        std::vector<int> level_off;  // refit plan: the nodes of height h are order[level_off[h] .. level_off[h + 1])
        std::vector<float> leaf_box; // [n_world][6], host side of d_leaf_box
        int *d_order = nullptr;      // node indices sorted by height
        float *d_leaf_box = nullptr;
        size_t bytes = 0;            // of the two device tables (part of device_bytes)
        hipEvent_t ev0 = nullptr, ev1 = nullptr; // RTMI_FLAG_TIMING: around the refit launches of the last in-place edit (rtmi_scene_last_refit_ms)
        bool timed = false;
    } geo;
    // the caller's arrays, copied at creation (the library keeps no host POINTERS): what rtmi_scene_clone replicates
    struct Args {
        std::vector<int32_t> prim_kind, prim_mat, mat_kind, mat_tex, tex_kind, tex_child, prim_flip, prim_xform, xform_kind, perm, media_calls, media_lo, image_wh;
        std::vector<double> prim_geom, mat_param, tex_param, cam, xform_param, perlin_vec;
        std::vector<uint8_t> image_rgb;
        int cam_kind = 0;
        int media_mode = 0;
        bool has_media_calls = false;
    } args;
};

namespace {

bool ctx_ok(rtmi_ctx *c) { return c && c->magic == 0x52544d49u; }
bool scene_ok(rtmi_scene *s) { return s && s->magic == 0x52545343u && ctx_ok(s->ctx); }
std::atomic<uint64_t> g_scene_serial{0}; // rtmi_scene::serial

// one scene table: its host copy and the DevScene field that receives its device address
struct Table {
    const void *data; size_t bytes, elem; const void **field;
    template <typename T> Table(const std::vector<T> &v, const T **f) : data(v.data()), bytes(v.size() * sizeof(T)), elem(sizeof(T)), field(reinterpret_cast<const void **>(f)) {}
};
int upload_to(std::vector<void *> &allocs, size_t &bytes, const Table &t) { // (an empty table still gets one element)
    void *p = nullptr;
    const size_t alloc = std::max(t.bytes, t.elem);
    if (hipMalloc(&p, alloc) != hipSuccess) return fail(RTMI_E_NOMEM, "hipMalloc(%zu) failed", alloc);
    allocs.push_back(p);
    bytes += alloc;
    if (t.bytes) HIP_TRY(hipMemcpy(p, t.data, t.bytes, hipMemcpyHostToDevice));
    *t.field = p;
    return RTMI_OK;
}
int upload(rtmi_scene *s, const Table &t) { return upload_to(s->allocs, s->device_bytes, t); }
// The tables of a packed scene, uploaded in the order they always were; their device addresses go into d (= the descriptor that P.d was copied to).
int upload_tables(const PackedScene &P, DevScene &d, std::vector<void *> &allocs, size_t &bytes) {
    const Table tables[] = {
        {P.stat_geom, &d.stat_geom}, {P.stat_orig, &d.stat_orig}, {P.bvh_nodes, &d.bvh_nodes}, {P.grid_cells, &d.grid_cells}, {P.moving_all, &d.moving_all},
        {P.leaf_rec, &d.leaf_rec}, {P.ext_info, &d.ext_info}, {P.ext_xf, &d.ext_xf}, {P.cull20, &d.cull20}, {P.exact12, &d.exact12}, {P.stat4_d, &d.stat4_d},
        {P.stat4_f, &d.stat4_f}, {P.mov_geom, &d.mov_geom}, {P.mov_orig, &d.mov_orig}, {P.M.prim_kind, &d.prim_kind}, {P.M.prim_km, &d.prim_km},
        {P.M.mat_rec, &d.mat_rec}, {P.M.mat_grad, &d.mat_grad}, {P.M.prim_mat, &d.prim_mat}, {P.M.mat_kind, &d.mat_kind}, {P.M.mat_tex, &d.mat_tex},
        {P.M.mat_param, &d.mat_param}, {P.M.tex_kind, &d.tex_kind}, {P.M.tex_param, &d.tex_param}, {P.M.tex_child, &d.tex_child}};
    for (const Table &t : tables) { const int rc = upload_to(allocs, bytes, t); if (rc) return rc; }
    return RTMI_OK;
}

// LDS tiling of the static spheres for a given precision
void lds_plan(const rtmi_ctx *c, int n_static, size_t real_bytes, int *prims_per_tile, int *n_ptiles, size_t *lds_bytes) {
    const size_t rec = 4 * real_bytes;
    int cap = (int)((size_t)c->max_lds_bytes / rec);
    int ppt = std::max(1, std::min(std::max(n_static, 1), cap));
    *prims_per_tile = ppt;
    *n_ptiles = std::max(1, (n_static + ppt - 1) / ppt);
    *lds_bytes = (size_t)ppt * rec + 16;
}

int tiles_x_of(int nx) { return (nx + RTMI_TILE - 1) / RTMI_TILE; }
int tiles_y_of(int ny) { return (ny + RTMI_TILE - 1) / RTMI_TILE; }

// Local tile list of a render: global tiles first, first+stride, ... that intersect the output region rg = {x0, y0, x1, y1}.
int ensure_tile_ids(rtmi_ctx *c, int nx, int ny, int first, int stride, const int *rg, hipStream_t st, int *n_local) {
    const int ntiles = tiles_x_of(nx) * tiles_y_of(ny);
    const int key[8] = {nx, ny, first, stride, rg[0], rg[1], rg[2], rg[3]};
    if (!std::memcmp(key, c->tile_key, sizeof key)) { *n_local = (int)c->tile_ids_host.size(); return RTMI_OK; }
    const int tx_n = tiles_x_of(nx);
    const bool whole = rg[0] <= 0 && rg[1] <= 0 && rg[2] >= nx && rg[3] >= ny;
    c->tile_ids_host.clear();
    long long valid = 0;
    for (int g = first; g < ntiles; g += stride) {
        const int px0 = (g % tx_n) * RTMI_TILE, py0 = (g / tx_n) * RTMI_TILE;
        const int ax0 = std::max(px0, rg[0]), ay0 = std::max(py0, rg[1]);
        const int ax1 = std::min(std::min(px0 + RTMI_TILE, nx), rg[2]), ay1 = std::min(std::min(py0 + RTMI_TILE, ny), rg[3]);
        if (ax1 <= ax0 || ay1 <= ay0) { if (whole) c->tile_ids_host.push_back(g); continue; } // (cannot happen for the whole frame)
        c->tile_ids_host.push_back(g);
        valid += (long long)(ax1 - ax0) * (ay1 - ay0);
    }
    const int nl = (int)c->tile_ids_host.size();
    *n_local = nl;
    c->tile_valid_pixels = valid;
    int rc = c->tile_ids.ensure((size_t)std::max(nl, 1) * sizeof(int));
    if (rc) return rc;
    if (nl) HIP_TRY(hipMemcpyAsync(c->tile_ids.p, c->tile_ids_host.data(), (size_t)nl * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st)); // tile_ids_host may be rewritten by the next call
    std::memcpy(c->tile_key, key, sizeof key);
    return RTMI_OK;
}

int next_event_pair(rtmi_ctx *c, hipEvent_t *a, hipEvent_t *b) {
    if (c->events_used == (int)c->events.size()) {
        hipEvent_t e0, e1;
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        c->events.emplace_back(e0, e1);
    }
    *a = c->events[(size_t)c->events_used].first;
    *b = c->events[(size_t)c->events_used].second;
    c->events_used++;
    return RTMI_OK;
}

// RTMI_FLAG_TIMING: the interval of one launch on `st`.  open_timed records its first event; *e1 = the event the caller records behind the kernel
// (null: not timed).  close_timed_fold records the event behind the fold that follows that kernel (rtmi_last_reduce_ms).
int open_timed(rtmi_ctx *c, hipStream_t st, hipEvent_t *e1) {
    hipEvent_t e0 = nullptr;
    *e1 = nullptr;
    if (!(c->flags & RTMI_FLAG_TIMING) || c->events_used >= 8192) return RTMI_OK;
    const int rc = next_event_pair(c, &e0, e1);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(e0, st));
    return RTMI_OK;
}
int close_timed_fold(rtmi_ctx *c, hipStream_t st) {
    const size_t k = (size_t)c->events_used - 1;
    while (c->events_r.size() <= k) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); c->events_r.push_back(e); }
    HIP_TRY(hipEventRecord(c->events_r[k], st));
    return RTMI_OK;
}

// Workgroups of `block` threads and lds_bytes of dynamic LDS that stay resident per CU.  The occupancy query is a runtime call per launch and
// replica: asked once per (kernel, LDS bytes) and kept on the context.
int resident_blocks(rtmi_ctx *c, const void *kern, int block, size_t lds_bytes, int *resident) {
    const std::pair<const void *, size_t> key(kern, lds_bytes);
    auto it = c->occupancy.find(key);
    if (it == c->occupancy.end()) {
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(resident, kern, block, lds_bytes));
        c->occupancy.emplace(key, *resident);
    } else *resident = it->second;
    return RTMI_OK;
}

// One launch on `st` of a persistent-queue kernel (rays_kernel, rays_nee_kernel, query_kernel) over `items` work items, and its timing interval:
// as many blocks as stay resident, none without an item, behind the zeroed queue head.  launch(grid, total_items, qblock) puts the two numbers into
// the kernel's argument struct and starts it.  fold() starts what reduces the kernel's output, if anything does: the interval's reduce part
// (rtmi_last_reduce_ms) ends behind it.
struct NoFold { void operator()() const {} };
template <typename Launch, typename Fold = NoFold>
int queue_launch(rtmi_ctx *c, hipStream_t st, const void *kern, size_t lds, unsigned *queue, long long items, Launch launch, Fold fold = Fold{}) {
    int resident = 0;
    const int rc = resident_blocks(c, kern, kBlock, lds, &resident);
    if (rc) return rc;
    const long long persistent = (long long)c->cus * std::max(1, std::min(c->blocks_per_cu, resident));
    // claim size: short claims on small launches (the tail matters), longer ones when a wave has many ahead of it
    const long long per_wave = items / std::max(1, c->cus * 16);
    unsigned qb = 64u;
    while (qb < 1024u && per_wave >= (long long)qb * 16) qb *= 2;
    hipEvent_t e1 = nullptr;
    const int rce = open_timed(c, st, &e1);
    if (rce) return rce;
    HIP_TRY(hipMemsetAsync(queue, 0, sizeof(unsigned), st));
    launch(dim3((unsigned)std::max<long long>(1, std::min<long long>(persistent, (items + kBlock - 1) / kBlock))), (unsigned)items, qb);
    HIP_TRY(hipGetLastError());
    if (e1) HIP_TRY(hipEventRecord(e1, st));
    fold();
    HIP_TRY(hipGetLastError());
    return e1 ? close_timed_fold(c, st) : RTMI_OK;
}

// the stream of a call: the caller's, or the context's own
hipStream_t stream_of(const rtmi_ctx *c, void *stream) { return stream ? reinterpret_cast<hipStream_t>(stream) : c->stream; }

// the output region [x0, x1) x [y0, y1) of a host form must lie inside the frame and hold a pixel
int check_region(int nx, int ny, int x0, int y0, int x1, int y1) {
    if (x0 < 0 || y0 < 0 || x1 > nx || y1 > ny || x1 <= x0 || y1 <= y0) return fail(RTMI_E_ARG, "region [%d,%d)x[%d,%d) outside %dx%d", x0, x1, y0, y1, nx, ny);
    return RTMI_OK;
}

// ---- which trace kernel a render launches --------------------------------------------------------------------------
// The launch knobs, read once per render call (null: not set).  RTMI_FLAT_BELOW / RTMI_SUSPEND_LANES override the options of the same names;
// RTMI_SPHERE_LDS_STASH=0 keeps the time-sliced sphere kernel's camera-ray stash in registers; RTMI_DEFER_EMITTERS overrides option "defer_emitters" (A/B runs).
struct LaunchKnobs { const char *flat_below, *suspend_lanes, *sphere_stash, *defer_emitters; };
LaunchKnobs read_launch_knobs() {
    return {std::getenv("RTMI_FLAT_BELOW"), std::getenv("RTMI_SUSPEND_LANES"), std::getenv("RTMI_SPHERE_LDS_STASH"), std::getenv("RTMI_DEFER_EMITTERS")};
}
// The material whose samples this render's fold finishes (TraceParams::defer_mat), -1: the render stores finished 3-real samples -- the scene has no
// deferred emitter (a mixed-kind scene never has), or the option / the knob says no
int launch_defer_mat(const rtmi_scene *s, const rtmi_ctx *c, const LaunchKnobs &k) {
    const bool on = k.defer_emitters ? k.defer_emitters[0] != '0' : c->defer_emitters != 0;
    return (on && !s->dev.has_ext) ? s->dev.defer_mat : -1;
}

// Dynamic LDS of a BVH kernel, per lane in words: `levels` stack columns, then `susp_words` of parked cursors (time-sliced instantiations), then
// `stash_words` of camera-ray stash; susp_off / stash_off are where the last two begin (TraceParams)
struct LdsLayout { int susp_off, stash_off; size_t bytes; };
LdsLayout lds_layout(int levels, int susp_words, int stash_words) {
    return {levels * RTMI_BVH_STRIDE, (levels + susp_words) * RTMI_BVH_STRIDE, (size_t)(levels + susp_words + stash_words) * kTraceBlock * sizeof(int)};
}

struct TracePlan {
    void (*kern)(ScenePtr, TraceParams) = nullptr;
    LdsLayout lds{RTMI_BVH_STACK * RTMI_BVH_STRIDE, 0, 0}; // (the sphere kernels' stack has the compile-time RTMI_BVH_STACK levels: immediate ds_ offsets)
    int suspend_lanes = 0;
    int accel = RTMI_ACCEL_BVH; // what runs: the request for the tree may be answered with the flat scan (rtmi_last_accel)
    bool defers = false;        // kern is a DEFER twin: the render stores 4-real records and its folds finish them
};

// The trace kernel of a render, its LDS layout and its time-slicing threshold.  multi / lds_bytes: the LDS tiling of the static spheres (lds_plan).
// defer_mat >= 0: the render may defer (launch_defer_mat) -- it does where the kernel has a DEFER twin: the tree kernels, traversal counters aside.
template <typename R>
TracePlan choose_trace_kernel(const rtmi_scene *s, const rtmi_ctx *c, const LaunchKnobs &k, bool multi, size_t lds_bytes, int defer_mat) {
    const DevScene &d = s->dev;
    TracePlan p;
    int variant = c->accel == RTMI_ACCEL_BVH ? SCAN_BVH : c->scan_variant;
    // a tree over a handful of mixed-kind primitives costs more than scanning them: a Cornell box's 18 (six of them too big for the tree anyway)
    // trace 8 % faster through the scalar-cache scan, the 3 - 8 of the small f3 / f4 scenes 3 - 10 %.  The two paths are bit-identical (tested
    // scene by scene), so the request for the tree is answered with the scan -- unless the tree's traversal counters were asked for.
    const int below = k.flat_below ? std::atoi(k.flat_below) : c->flat_below;
    if (variant == SCAN_BVH && d.has_ext && !c->count_traversal && d.n_all < below) variant = SCAN_SGPR_CULL;
    p.accel = variant == SCAN_BVH ? RTMI_ACCEL_BVH : RTMI_ACCEL_FLAT;
    const bool bvh = variant == SCAN_BVH, count = c->count_traversal != 0;
    p.suspend_lanes = c->suspend_lanes;
    if (d.has_ext && !c->suspend_lanes_set) p.suspend_lanes = 12; // make-final, 20 frames each, thresholds 8 / 10 / 12 / 14: 16.22 - 16.30 / 16.16 - 16.21 / 16.12 - 16.20 / 16.21 - 16.22 ms
    if (k.suspend_lanes) p.suspend_lanes = std::max(0, std::min(64, std::atoi(k.suspend_lanes)));
    // Stack columns for THIS scene's tree (its depth is known) and the camera-ray stash: 11 words per entry, 17 when the rays' origins differ
    const int levels = std::max(4, std::min(RTMI_BVH_STACK, s->bvh_depth + 2));
    const int stash_words = d.cam_fixed_origin ? 11 : 17;
    constexpr bool kExtLdsStash = RTMI_STASH && RTMI_EXT_LDS_STASH && !RTMI_EXT_NO_STASH;
    if (d.has_ext && d.media_seq) { // a Hitlist world holding media (RTMI_MEDIA_HITLIST): its own instantiations, never time-sliced
        const bool nar = d.media_seq == 2; // RTMI_MEDIA_NARROWED: Hitlists holding media below bvh-nodes (MSEQ = 2)
        if (bvh && nar) p.kern = count ? trace_kernel<double, false, SCAN_BVH, true, true, false, 2> : trace_kernel<double, false, SCAN_BVH, true, false, false, 2>;
        else if (bvh) p.kern = count ? trace_kernel<double, false, SCAN_BVH, true, true, false, 1> : trace_kernel<double, false, SCAN_BVH, true, false, false, 1>;
        else p.kern = nar ? trace_kernel<double, false, SCAN_SGPR_CULL, true, false, true, 2> : trace_kernel<double, false, SCAN_SGPR_CULL, true, false, true, 1>;
        p.lds = lds_layout(bvh ? levels : 0, 0, kExtLdsStash ? stash_words : 0);
    } else if (d.has_ext) { // section 8(f3) scenes: FP64 kernels with the mixed-kind intersectors
        // a Cornell box's 20-primitive tree loses 5 % to the time-slicing machinery, make-final's 3400 gain 8 %
        const bool slice = bvh && s->bvh_node_count >= 128 && p.suspend_lanes > 0;
        if (bvh && count) p.kern = slice ? trace_kernel<double, false, SCAN_BVH, true, true> : trace_kernel<double, false, SCAN_BVH, true, true, false>;
        else if (bvh) p.kern = slice ? trace_kernel<double, false, SCAN_BVH, true> : trace_kernel<double, false, SCAN_BVH, true, false, false>;
        else p.kern = trace_kernel<double, false, SCAN_SGPR_CULL, true>;
        p.lds = lds_layout(bvh ? levels : 0, slice ? RTMI_BVH_SUSPEND_WORDS_EXT : 0, kExtLdsStash ? stash_words : 0);
    } else if (bvh) {
        // suspend_lanes = 0 or a small tree (< 128 inner nodes) selects the instantiation without the time-slicing machinery (the plain while-while loop);
        // a scene with an entry grid always runs the time-sliced one (threshold 0 = never park early): the piecewise walk of long segments lives there
        const bool slice = (p.suspend_lanes > 0 && s->bvh_node_count >= 128) || d.grid_n > 0;
        p.lds.bytes = (size_t)(RTMI_BVH_STACK + RTMI_BVH_SUSPEND_WORDS) * kTraceBlock * sizeof(int); // stack columns + suspended cursors
        // The time-sliced sphere kernel keeps its camera-ray stash in LDS too when the scene's tree leaves room for it beside the stack columns (a dead lane reads
        // its entry with 6 ds_read instead of 11 ds_bpermute, and 14 VGPRs come free): C3 69.30 -> 68.76 ms, C2 3.067 -> 3.040 (RTMI_SPHERE_LDS_STASH=0: the
        // register stash, which deeper trees -- more than 21 levels with their grid entries -- keep anyway: a fifth kilobyte-row would cost the fourth workgroup per CU)
        const LdsLayout stash = lds_layout(levels, RTMI_BVH_SUSPEND_WORDS, stash_words);
        if (slice) p.kern = count ? trace_kernel<R, false, SCAN_BVH, false, true> : trace_kernel<R, false, SCAN_BVH>;
        else p.kern = count ? trace_kernel<R, false, SCAN_BVH, false, true, false> : trace_kernel<R, false, SCAN_BVH, false, false, false>;
        const bool lst = slice && !count && !(k.sphere_stash && k.sphere_stash[0] == '0') && stash.bytes <= 40 * 1024; // four workgroups per CU still fit
        if (lst) { p.kern = trace_kernel<R, false, SCAN_BVH, false, false, true, false, true>; p.lds = stash; }
        if (defer_mat >= 0 && !count) {
            p.defers = true;
            p.kern = lst ? trace_kernel<R, false, SCAN_BVH, false, false, true, 0, true, true>
                         : slice ? trace_kernel<R, false, SCAN_BVH, false, false, true, 0, false, true> : trace_kernel<R, false, SCAN_BVH, false, false, false, 0, false, true>;
        }
    } else if (variant == SCAN_SGPR_CULL) p.kern = trace_kernel<R, false, SCAN_SGPR_CULL>;
    else if (variant == SCAN_SGPR) p.kern = trace_kernel<R, false, SCAN_SGPR>;
    else {
        p.kern = variant == SCAN_LDS_PIPE ? (multi ? trace_kernel<R, true, SCAN_LDS_PIPE> : trace_kernel<R, false, SCAN_LDS_PIPE>)
                                          : (multi ? trace_kernel<R, true, SCAN_LDS_LITERAL> : trace_kernel<R, false, SCAN_LDS_LITERAL>);
        p.lds.bytes = lds_bytes;
    }
    return p;
}

#ifdef RTMI_STAMPS
// diagnostic build only (make stamps): the in-kernel phase stamps of the last trace launch, reported on stderr and cleared
int report_phase_stamps(rtmi_ctx *c, hipStream_t st) {
    const int grid_trace_dbg = c->last_grid;
    HIP_TRY(hipStreamSynchronize(st));
    unsigned long long h[3 * PH_SLOTS] = {0}, z[3 * PH_SLOTS] = {0};
    HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_phase), sizeof(h)));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof(z)));
    {
        static unsigned long long wt[2][4096];
        HIP_TRY(hipMemcpyFromSymbol(wt, HIP_SYMBOL(g_wg_t), sizeof(wt)));
        const int g = std::min(4096, grid_trace_dbg);
        unsigned long long t0 = ~0ull; for (int k = 0; k < g; ++k) t0 = std::min(t0, wt[0][k]);
        std::vector<double> e(g), b(g); for (int k = 0; k < g; ++k) { e[k] = (wt[1][k] - t0) * 1e-5; b[k] = (wt[0][k] - t0) * 1e-5; }
        std::sort(e.begin(), e.end()); std::sort(b.begin(), b.end());
        fprintf(stderr, "[stamps] workgroup start (ms after first): median %.3f max %.3f | end: min %.3f p10 %.3f median %.3f p90 %.3f max %.3f (last pass, %d workgroups)\n",
                b[g / 2], b[g - 1], e[0], e[g / 10], e[g / 2], e[g * 9 / 10], e[g - 1], g);
    }
    static const char *names[PH_N] = {"loop/tail", "refill: generate (stash write)", "refill: claim + deal", "bvh: ray setup / resume", "bvh: big primitives (exact)",
                                      "bvh: descent (node visits)", "bvh: leaf exact tests", "bvh: loop control / park", "shade: hit record", "shade: |d| normalise",
                                      "shade: rand-in-unit-sphere", "shade: material record + directions", "shade: texture", "shade: store / rest", "shade: sphere uv", "(stamp calibration)",
                                      "bvh: grid entry / next piece of the walk", "media: chords, draws, log", "generate: key, jitter, u v", "generate: lens disk rounds",
                                      "generate: camera arithmetic", "grid entry: box ranges, ray constants", "grid entry: the rectangle", "grid entry: start cell, piece end",
                                      "roots: second-root arm (big primitives)", "roots: second-root arm (leaf)"};
    // every interval begins with the bookkeeping of the stamp that opened it: subtract the cost of one stamp (PH_CAL: back-to-back stamps) per stamp
    const double per_stamp = h[2 * PH_SLOTS + PH_CAL] ? (double)h[PH_CAL] / (double)h[2 * PH_SLOTS + PH_CAL] : 0.0;
    double tk[PH_N], lk[PH_N], tot = 0, totl = 0, raw = 0;
    for (int k = 0; k < PH_N; ++k) {
        raw += (double)h[k];
        const double t = (double)h[k], c = std::min(t, per_stamp * (double)h[2 * PH_SLOTS + k]);
        tk[k] = k == PH_CAL ? 0.0 : t - c;
        lk[k] = t > 0 ? (double)h[PH_SLOTS + k] * (tk[k] / t) : 0.0;
        tot += tk[k]; totl += lk[k];
    }
    fprintf(stderr, "[phases] one stamp = %.0f ticks; stamps took %.1f %% of the %.4g wave-ticks of this (diagnostic) launch and are subtracted below\n", per_stamp, 100 * (raw - tot) / raw, raw);
    fprintf(stderr, "[phases] %-36s %8s %8s %10s %10s %12s\n", "phase", "ticks %", "lanes", "masked %", "useful %", "stamps");
    for (int k = 0; k < PH_N; ++k) {
        if (!h[k] || k == PH_CAL) continue;
        const double t = tk[k], l = lk[k];
        fprintf(stderr, "[phases] %-36s %8.2f %8.1f %10.2f %10.2f %12llu\n", names[k], 100 * t / tot, t > 0 ? l / t : 0.0, 100 * (64 * t - l) / (64 * tot), 100 * l / (64 * tot), h[2 * PH_SLOTS + k]);
    }
    fprintf(stderr, "[phases] %-36s %8.2f %8.1f %10.2f %10.2f   (%.4g wave-ticks)\n", "total", 100.0, totl / tot, 100 * (64 * tot - totl) / (64 * tot), 100 * totl / (64 * tot), tot);
    return RTMI_OK;
}
#endif

// f(double{}) or f(float{}): a call's precision selects the instantiation
template <typename F> auto with_real(int precision, F f) { return precision == RTMI_F64 ? f(double{}) : f(float{}); }

// the output region rg = {x0, y0, x1, y1} clipped to the image
struct Region { int x0, y0, x1, y1; };
Region clip_region(const int *rg, int nx, int ny) { return {std::max(rg[0], 0), std::max(rg[1], 0), std::min(rg[2], nx), std::min(rg[3], ny)}; }

// adaptive_compact_kernel on `st`.  tile_ids != null: the identity over a render's n tiles into list 0, n_t = init_n_t everywhere (the start of the
// per-tile state); tile_ids = null: the n entries of the frame's current list, filtered by `keep`, into the other list.  The list written is current.
hipError_t launch_compact(ProgFrame &f, const int *tile_ids, int n, int init_n_t, int tiles_x, const Region &r, hipStream_t st) {
    const bool start = tile_ids != nullptr;
    const int to = start ? 0 : 1 - f.cur;
    hipLaunchKernelGGL(adaptive_compact_kernel, dim3(1), dim3(kCompactBlock), 0, st, start ? nullptr : reinterpret_cast<const int *>(f.keep.p),
                       start ? tile_ids : reinterpret_cast<const int *>(f.act_tiles[f.cur].p),
                       start ? nullptr : reinterpret_cast<const int *>(f.act_slots[f.cur].p), n, reinterpret_cast<int *>(f.act_tiles[to].p),
                       reinterpret_cast<int *>(f.act_slots[to].p), reinterpret_cast<int *>(f.meta.p), start ? init_n_t : -1,
                       start ? reinterpret_cast<int *>(f.n_t.p) : nullptr, tiles_x, r.x0, r.y0, r.x1, r.y1);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) f.cur = to;
    return e;
}

// The per-tile state of a frame whose n_local tiles (tile_ids, the context's tile list) all hold k samples and are all active: the arrays, the
// identity compaction with n_t = k, the host's mirror.  A launch failure is reported as "`what`: ..." with RTMI_E_DEVICE.
int ensure_tile_state(ProgFrame &f, const int *tile_ids, int n_local, int k, int tiles_x, const Region &r, hipStream_t st, const char *what) {
    const size_t ints = (size_t)std::max(n_local, 1) * sizeof(int);
    int rc = RTMI_OK;
    for (int i = 0; i < 2 && !rc; ++i) { rc = f.act_tiles[i].ensure(ints); if (!rc) rc = f.act_slots[i].ensure(ints); }
    if (!rc) rc = f.n_t.ensure(ints);
    if (!rc) rc = f.keep.ensure(ints);
    if (!rc) rc = f.meta.ensure(2 * sizeof(int));
    if (rc) return rc;
    const hipError_t e = launch_compact(f, tile_ids, n_local, k, tiles_x, r, st);
    if (e != hipSuccess) return fail(RTMI_E_DEVICE, "%s: %s", what, hipGetErrorString(e));
    f.adaptive = true;
    f.n_active = n_local; f.active_pixels = f.valid_pixels;
    f.pixel_samples = f.valid_pixels * (long long)k;
    return RTMI_OK;
}

// render_passes, step 1 (progressive and adaptive calls): the frame for this call.  A new frame (s_first = 0) gets its buffers, real_bytes per sum,
// and zeroed counters; a continuation's are checked; an adaptive call (ad) on a frame without per-tile state builds it.  From here on the frame is
// being changed: it only holds samples again (k > 0) once the call has succeeded.
int prepare_frame(rtmi_ctx *c, ProgFrame *prog, const AdaptiveCall *ad, int n_local, int s_first, size_t real_bytes, int tiles_x, const Region &r,
                  hipStream_t st) {
    prog->k = 0;
    const size_t elems = (size_t)std::max(n_local, 1) * 192;
    if (s_first == 0) {
        int rc = prog->sums.ensure(elems * real_bytes);
        if (!rc) rc = prog->mean.ensure(elems * sizeof(double));
        if (!rc) rc = prog->m2.ensure(elems * sizeof(double));
        if (!rc) rc = prog->counters.ensure(2 * sizeof(u64));
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(prog->counters.p, 0, 2 * sizeof(u64), st));
    } else if (prog->sums.bytes < elems * real_bytes || prog->m2.bytes < elems * sizeof(double)) {
        return fail(RTMI_E_STATE, "progressive frame buffers do not match the frame"); // (the key check makes this unreachable)
    }
    if (s_first == 0 || !ad) prog->adaptive = false; // a new frame, or a uniform continuation (no tile retired: the entries checked): every tile active, n_t = k
    prog->n_tiles = n_local; prog->valid_pixels = c->tile_valid_pixels;
    if (ad && !prog->adaptive) // the per-tile state of a frame whose tiles all hold ad->k_before samples (0: a new frame) and are all active
        return ensure_tile_state(*prog, reinterpret_cast<const int *>(c->tile_ids.p), n_local, ad->k_before, tiles_x, r, st, "hipGetLastError()");
    return RTMI_OK;
}

// render_passes, step 2: how many of the call's ns samples of n_local tiles one pass takes, and a sample buffer that holds them.
// record_reals: 3, or 4 for a render that defers.  The BUDGET counts 3 reals per item either way -- the split of a call into passes does not depend on
// option "defer_emitters" --; the buffer, the free-HBM clamp and the halving retry take the record as it is, the fourth real on top of the budget.
int size_sample_passes(rtmi_ctx *c, int n_local, int ns, size_t real_bytes, int record_reals, int *out_s_per_pass) {
    const size_t budgeted = (size_t)n_local * 64 * 3 * real_bytes;
    const size_t per_sample = (size_t)n_local * 64 * (size_t)record_reals * real_bytes;
    int s_per_pass = (int)std::max<int64_t>(1, std::min<int64_t>(ns, c->workspace_bytes / (int64_t)budgeted));
    // the work queue is indexed with 32 bits: items per pass (+ one claim per wave past the end) must stay below 2^32
    while (s_per_pass > 1 && (long long)n_local * s_per_pass * 64 >= 0xf0000000ll) s_per_pass /= 2;
    if ((long long)n_local * s_per_pass * 64 >= 0xf0000000ll) return fail(RTMI_E_ARG, "frame too large for one pass: %d tiles per rank", n_local);
    if (per_sample * (size_t)s_per_pass > c->samples.bytes) {
        // The buffer has to grow.  The budget is what the option allows AND what the device can give: at most kFreeShare of the HBM that
        // is free right now (plus what this context's buffer already holds) -- a host that shares the GPU (PyTorch's caching allocator, a
        // second render slot) gets more passes instead of RTMI_E_NOMEM.  If the allocation still fails, halve the pass and retry.
        constexpr double kFreeShare = 0.8;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const double avail = kFreeShare * (double)free_b + (double)c->samples.bytes;
            const int fit = (int)std::max<double>(1.0, std::min<double>((double)s_per_pass, avail / (double)per_sample));
            s_per_pass = std::min(s_per_pass, fit);
        }
        for (;;) {
            int rc;
            if (c->fail_allocs > 0) { c->fail_allocs--; c->samples.release(); rc = fail(RTMI_E_NOMEM, "hipMalloc(%zu bytes) failed (injected by the test hook)", per_sample * (size_t)s_per_pass); }
            else rc = c->samples.ensure(per_sample * (size_t)s_per_pass);
            if (!rc) break;
            (void)hipGetLastError(); // a failed hipMalloc leaves its error sticky
            if (s_per_pass == 1) return rc;
            s_per_pass = (s_per_pass + 1) / 2;
        }
    }
    *out_s_per_pass = s_per_pass;
    return RTMI_OK;
}

// render_passes, step 3: one trace launch on `st`.  tp holds what the call fixes; the pass adds its samples [s_begin, s_begin + s_count), the
// claim size and a zeroed queue head.  *out_e1 = the timing event behind the kernel (null: not timed).
int launch_trace_pass(rtmi_scene *s, const TracePlan &plan, TraceParams &tp, int s_begin, int s_count, hipStream_t st, hipEvent_t *out_e1) {
    rtmi_ctx *c = s->ctx;
    tp.s_begin = s_begin; tp.s_count = s_count;
    hipEvent_t e1 = nullptr;
    int rc = open_timed(c, st, &e1);
    if (rc) return rc;
    tp.total_items = (unsigned)((long long)tp.n_local_tiles * s_count * 64);
    { // claim size: one global atomic per claim -- 256 items on small launches (a short tail matters more), up to 1024 when a wave has
      // thousands of claims ahead of it (C3: 129 000 items per wave)
        const long long per_wave = (long long)tp.total_items / std::max(1, c->cus * 16);
        // (mixed-kind scenes: 192 -- their launches are short and end in a long die-off of deep paths through the media; make-final 64 / 128 / 192 / 256 / 320 / 384 / 512 items:
        // 18.2 / 17.3 / 17.1 - 17.2 / 17.4 - 17.5 / 17.9 / 18.3 / 19.4 ms, the Cornell box indifferent)
        unsigned qb = s->dev.has_ext ? 192u : kQueueBlock;
        while (qb < 1024u && per_wave >= (long long)qb * 128) qb *= 2;
        if (const char *e = std::getenv("RTMI_QUEUE_BLOCK_RT")) qb = std::max(64, std::atoi(e) / 64 * 64);
        tp.qblock = qb;
    }
    HIP_TRY(hipMemsetAsync(tp.queue, 0, sizeof(unsigned), st));
    // persistent launch: as many workgroups as stay resident (at most blocks_per_cu per CU); the queue feeds them
    int resident = 0;
    rc = resident_blocks(c, reinterpret_cast<const void *>(plan.kern), kTraceBlock, plan.lds.bytes, &resident);
    if (rc) return rc;
    const int grid_trace = std::max(1, c->cus * std::max(1, std::min(c->blocks_per_cu * (256 / kTraceBlock), resident)));
    if (c->last_grid != grid_trace && std::getenv("RTMI_DEBUG"))
        fprintf(stderr, "[rtmi] trace launch: %d workgroups of %d threads (%d resident per CU by the occupancy query, cap %d), %zu B LDS each\n",
                grid_trace, kTraceBlock, resident, c->blocks_per_cu * (256 / kTraceBlock), plan.lds.bytes);
    c->last_grid = grid_trace;
    hipLaunchKernelGGL(plan.kern, dim3(grid_trace), dim3(kTraceBlock), plan.lds.bytes, st, s->d_dev, tp);
    HIP_TRY(hipGetLastError());
    if (e1) HIP_TRY(hipEventRecord(e1, st));
    *out_e1 = e1;
    return RTMI_OK;
}

// render_passes, step 4: the fold of the pass tp traced.  A one-shot render (prog = null): reduce_kernel into c->accum and, on the last of the ns
// samples, the mean into d_tiles_linear; a progressive call: frame_fold_kernel into the frame; an adaptive one (ad): its retiring instantiation,
// which decides on the pass that ends at s_end.  Timed (e1): the fold is the interval from the trace kernel's end event to one recorded here.
template <typename R>
int launch_fold(rtmi_ctx *c, const TraceParams &tp, const double *defer_grad, int ns, int s_end, void *d_tiles_linear, bool count_pixels, ProgFrame *prog,
                const AdaptiveCall *ad, hipEvent_t e1, hipStream_t st) {
    const long long npx = (long long)tp.n_local_tiles * 64;
    const dim3 grid((unsigned)((npx + kBlock - 1) / kBlock));
    const R *samples = reinterpret_cast<const R *>(c->samples.p);
    const bool defer = tp.defer_mat >= 0; // the pass was traced into 4-real records: the DEFER twins
    if (ad) {
        FoldRetire rt;
        rt.act_slots = reinterpret_cast<const int *>(prog->act_slots[prog->cur].p);
        rt.last = tp.s_begin + tp.s_count == s_end ? 1 : 0; rt.eps = ad->eps;
        rt.keep = reinterpret_cast<int *>(prog->keep.p); rt.n_t = reinterpret_cast<int *>(prog->n_t.p);
        hipLaunchKernelGGL((defer ? frame_fold_kernel<R, true, true> : frame_fold_kernel<R, true>), grid, dim3(kBlock), 0, st, samples, reinterpret_cast<R *>(prog->sums.p),
                           reinterpret_cast<double *>(prog->mean.p), reinterpret_cast<double *>(prog->m2.p), tp.tile_ids, tp.tiles_x, tp.n_local_tiles,
                           tp.s_begin, tp.s_count, tp.counters, (u64)c->tile_valid_pixels, tp.rx0, tp.ry0, tp.rx1, tp.ry1, rt, defer_grad);
    } else if (prog)
        hipLaunchKernelGGL((defer ? frame_fold_kernel<R, false, true> : frame_fold_kernel<R, false>), grid, dim3(kBlock), 0, st, samples, reinterpret_cast<R *>(prog->sums.p),
                           reinterpret_cast<double *>(prog->mean.p), reinterpret_cast<double *>(prog->m2.p), tp.tile_ids, tp.tiles_x, tp.n_local_tiles,
                           tp.s_begin, tp.s_count, tp.counters, (u64)c->tile_valid_pixels, tp.rx0, tp.ry0, tp.rx1, tp.ry1, FoldRetire{}, defer_grad);
    else
        hipLaunchKernelGGL((defer ? reduce_kernel<R, true> : reduce_kernel<R>), grid, dim3(kBlock), 0, st, samples, reinterpret_cast<R *>(c->accum.p),
                           reinterpret_cast<double *>(d_tiles_linear), tp.tile_ids, tp.tiles_x, tp.nx, tp.ny, tp.n_local_tiles, tp.s_begin, tp.s_count, ns,
                           count_pixels ? tp.counters : nullptr, (u64)c->tile_valid_pixels, tp.rx0, tp.ry0, tp.rx1, tp.ry1, defer_grad);
    HIP_TRY(hipGetLastError());
    return e1 ? close_timed_fold(c, st) : RTMI_OK;
}

// The sample passes of a render: samples [s_first, s_end) of every pixel of the local tiles, as many per pass as the sample buffer holds, each pass one
// trace launch followed by its fold.  A one-shot render (prog = null) runs samples [0, ns) and reduce_kernel folds them into c->accum and, on the last
// pass, the mean into d_tiles_linear.  A progressive call (prog = the context's frame) folds them into the frame with frame_fold_kernel; the trace
// kernel counts its rays into the frame's counters.  An adaptive call (ad) traces and folds the frame's active list and ends with the compaction that
// retires tiles.  A progressive call that fails once it got past the test hook has dropped its frame (k = 0).
template <typename R>
int render_passes(rtmi_scene *s, int nx, int ny, int s_first, int s_end, int depth, uint64_t seed, int first, int stride, const int *rg, void *d_tiles_linear,
                  void *d_counters, hipStream_t st, ProgFrame *prog, const AdaptiveCall *ad = nullptr) {
    rtmi_ctx *c = s->ctx;
    int n_local = 0;
    const int whole[4] = {0, 0, nx, ny};
    if (!rg) rg = whole;
    const Region region = clip_region(rg, nx, ny);
    int rc = ensure_tile_ids(c, nx, ny, first, stride, rg, st, &n_local);
    if (rc) return rc;
    c->last_stream = st;
    if (c->fail_next_render) { c->fail_next_render = 0; return fail(RTMI_E_DEVICE, "render failed (injected by the test hook test_fail_next_render)"); }
    if (prog) {
        rc = prepare_frame(c, prog, ad, n_local, s_first, sizeof(R), tiles_x_of(nx), region, st);
        if (rc) return rc;
        d_counters = prog->counters.p;
    }
    rc = c->counters.ensure(8 * sizeof(u64)); // [0..1] the metrics when the caller passes no buffer, [2] the work-queue head, [3..4] traversal counters
    if (rc) return rc;
    if (d_counters && !prog) HIP_TRY(hipMemsetAsync(d_counters, 0, 2 * sizeof(u64), st));
    HIP_TRY(hipMemsetAsync(reinterpret_cast<u64 *>(c->counters.p) + 3, 0, 2 * sizeof(u64), st));
    if (n_local == 0) { if (prog) { prog->k = s_end; c->last_passes = 0; } return RTMI_OK; } // (a dealt frame on a rank beyond the last tile: an empty frame that still counts its calls)
    if (ad) n_local = prog->n_active; // an adaptive call traces and folds the frame's active list, not the render's tile list
    if (n_local == 0) { prog->k = s_end; c->last_passes = 0; return RTMI_OK; } // every tile has retired: nothing to trace, k advances

    const int ns = s_end - s_first; // samples this call renders
    int s_per_pass = 0;
    const LaunchKnobs knobs = read_launch_knobs();
    int ppt, nptiles;
    size_t lds_bytes;
    lds_plan(c, s->dev.n_static, sizeof(R), &ppt, &nptiles, &lds_bytes);
    const TracePlan plan = choose_trace_kernel<R>(s, c, knobs, nptiles > 1, lds_bytes, launch_defer_mat(s, c, knobs));
    const int defer_mat = plan.defers ? s->dev.defer_mat : -1;
    rc = size_sample_passes(c, n_local, ns, sizeof(R), defer_mat >= 0 ? 4 : 3, &s_per_pass);
    if (rc) return rc;
    c->last_accel = plan.accel;
    c->last_record_reals = defer_mat >= 0 ? 4 : 3;
    c->last_passes = (ns + s_per_pass - 1) / s_per_pass;
    if (!prog && s_per_pass < ns) {
        rc = c->accum.ensure((size_t)n_local * 64 * 3 * sizeof(R));
        if (rc) return rc;
    }

    TraceParams tp; // what every pass of the call shares; launch_trace_pass adds the pass
    tp.nx = nx; tp.ny = ny; tp.depth = depth; tp.seed = seed; tp.tiles_x = tiles_x_of(nx);
    tp.n_local_tiles = n_local;
    tp.tile_ids = ad ? reinterpret_cast<const int *>(prog->act_tiles[prog->cur].p) : reinterpret_cast<const int *>(c->tile_ids.p);
    tp.samples = c->samples.p;
    tp.counters = d_counters ? reinterpret_cast<u64 *>(d_counters) : reinterpret_cast<u64 *>(c->counters.p);
    tp.prims_per_tile = (c->scan_variant >= SCAN_SGPR || s->dev.has_ext) ? 0 : ppt; tp.n_ptiles = nptiles;
    tp.queue = reinterpret_cast<unsigned *>(reinterpret_cast<u64 *>(c->counters.p) + 2);
    tp.rx0 = region.x0; tp.ry0 = region.y0; tp.rx1 = region.x1; tp.ry1 = region.y1;
    tp.trav = reinterpret_cast<u64 *>(c->counters.p) + 3;
    tp.suspend_lanes = plan.suspend_lanes; tp.susp_off = plan.lds.susp_off; tp.stash_off = plan.lds.stash_off;
    tp.rnx = 1.0 / (double)nx; tp.rny = 1.0 / (double)ny; tp.fixed_rays = camera_fixed_rays(s->dev.cam_kind, s->dev.cam_fixed_origin, s->dev.cam);
    tp.defer_mat = defer_mat;
    const double *defer_grad = defer_mat >= 0 ? s->dev.mat_grad + (size_t)defer_mat * 12 : nullptr; // the DEFER folds' operand
    for (int s_begin = s_first; s_begin < s_end; s_begin += s_per_pass) {
        hipEvent_t e1 = nullptr;
        rc = launch_trace_pass(s, plan, tp, s_begin, std::min(s_per_pass, s_end - s_begin), st, &e1);
        if (!rc) rc = launch_fold<R>(c, tp, defer_grad, ns, s_end, d_tiles_linear, d_counters != nullptr, prog, ad, e1, st);
        if (rc) return rc;
    }
#ifdef RTMI_STAMPS
    rc = report_phase_stamps(c, st);
#endif
    if (!rc && ad) // retire: the next active list, in tile order, and its length for the host
        HIP_TRY(launch_compact(*prog, nullptr, n_local, -1, tiles_x_of(nx), region, st));
    if (!rc && prog) prog->k = s_end;
    return rc;
}

template <typename R>
int render_tiles_impl(rtmi_scene *s, int nx, int ny, int ns, int depth, uint64_t seed, int first, int stride, const int *rg, void *d_tiles_linear,
                      void *d_counters, hipStream_t st) {
    return render_passes<R>(s, nx, ny, 0, ns, depth, seed, first, stride, rg, d_tiles_linear, d_counters, st, nullptr);
}

int check_render_args(rtmi_scene *s, int nx, int ny, int ns, int depth, int precision) {
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    if (nx <= 0 || ny <= 0 || ns <= 0 || depth < 0) return fail(RTMI_E_ARG, "nx, ny, ns must be > 0 and depth >= 0 (got %d %d %d %d)", nx, ny, ns, depth);
    if ((long long)nx * ny > (1ll << 30)) return fail(RTMI_E_ARG, "frame too large");
    if (precision != RTMI_F64 && precision != RTMI_F32) return fail(RTMI_E_ARG, "precision must be RTMI_F64 or RTMI_F32");
    if (precision == RTMI_F32 && s->dev.has_ext) return fail(RTMI_E_UNSUPPORTED, "rectangles / triangles / instances / procedural textures are rendered by the FP64 kernels only");
    if (s->uses_perlin && !s->have_perlin) return fail(RTMI_E_STATE, "the scene holds a Perlin texture: call rtmi_scene_set_perlin first");
    if (s->max_image >= s->dev.n_images) return fail(RTMI_E_STATE, "the scene holds an ImageMap with index %d: call rtmi_scene_set_images first", s->max_image);
    return RTMI_OK;
}

// The host forms' staging.  A call names its planes -- element count and the host arrays to copy from (`up`) and to (`down`), either or both null --
// then reserve() lays them out in c->io, every plane on a multiple of 16 bytes whatever the order, and hands out the device pointers.  A plane that
// is not present takes no space and its device pointer is null: what the *_impl functions take for "not given".  upload() and download() synchronise
// the context's stream once and copy every present plane that has a host array on that side; they return the first HIP error, so each entry keeps
// its own failure action.
struct IoPlane { size_t elem, count; bool present; const void *up; void *down; void **dev; size_t off; };

// where each plane starts (IoPlane::off); returns the bytes the arena needs
size_t io_layout(IoPlane *pl, int n) {
    size_t at = 0;
    for (int i = 0; i < n; ++i) { pl[i].off = at; if (pl[i].present) at += (pl[i].elem * pl[i].count + 15) & ~(size_t)15; }
    return at;
}

struct HostIo {
    rtmi_ctx *c;
    IoPlane pl[16]; // (rtmi_reproject names twelve)
    int n = 0;
    explicit HostIo(rtmi_ctx *ctx) : c(ctx) {}
    template <typename T> void plane(T **dev, size_t count, bool present, const void *up, void *down) { pl[n++] = {sizeof(T), count, present, up, down, reinterpret_cast<void **>(dev), 0}; }
    template <typename T> void in(T **dev, size_t count, const void *host) { plane(dev, count, host != nullptr, host, nullptr); } // an input, optional
    template <typename T> void out(T **dev, size_t count, void *host) { plane(dev, count, host != nullptr, nullptr, host); }     // an output, optional
    template <typename T> void work(T **dev, size_t count, void *host) { plane(dev, count, true, nullptr, host); } // the device side needs it; copied back where asked for
    int reserve() {
        const int rc = c->io.ensure(io_layout(pl, n));
        for (int i = 0; i < n && !rc; ++i) *pl[i].dev = pl[i].present ? static_cast<char *>(c->io.p) + pl[i].off : nullptr;
        return rc;
    }
    hipError_t copy(bool up) const {
        hipError_t e = hipStreamSynchronize(c->stream);
        for (int i = 0; i < n && e == hipSuccess; ++i) {
            const IoPlane &p = pl[i];
            if (p.present && up && p.up) e = hipMemcpy(*p.dev, p.up, p.elem * p.count, hipMemcpyHostToDevice);
            if (p.present && !up && p.down) e = hipMemcpy(p.down, *p.dev, p.elem * p.count, hipMemcpyDeviceToHost);
        }
        return e;
    }
    hipError_t upload() const { return copy(true); }
    hipError_t download() const { return copy(false); }
    // the entries without a failure action of their own: reserve() and upload() before the launches, download() behind them
    int stage() { const int rc = reserve(); if (rc) return rc; HIP_TRY(upload()); return RTMI_OK; }
    int finish() const { HIP_TRY(hipGetLastError()); HIP_TRY(download()); return RTMI_OK; }
};

// The two forms of an entry differ in where its planes lie.  What they share -- the checks, the light table, hipSetDevice -- is the family's
// *_begin, and the launches are its *_run or *_impl, which takes device pointers and a stream.  A _device form casts the caller's pointers
// (as<T>) and takes the caller's stream (stream_of); a host form names its planes in a HostIo and hands the launches to host_run: the inputs go
// up, launches(stream) queues the call on the context's stream, the outputs come back.
template <typename T, typename V> T *as(V *p) { return reinterpret_cast<T *>(p); }
template <typename Launches> int host_run(HostIo &io, Launches launches) {
    int rc = io.stage();
    if (!rc) rc = launches(io.c->stream);
    return rc ? rc : io.finish();
}
// A host state that continues an estimate (first > 0) holds `first` in every record's count, slot `at` of `stride` doubles; the message names
// the records ("group") and what they count, as the header's argument is called ("rays, g_first")
int check_state_counts(const double *state, size_t n, int stride, int at, int first, const char *noun, const char *counted) {
    if (state && first > 0)
        for (size_t g = 0; g < n; ++g)
            if (state[g * stride + at] != (double)first)
                return fail(RTMI_E_STATE, "%s %zu's record holds %g %s is %d", noun, g, state[g * stride + at], counted, first);
    return RTMI_OK;
}

// The planes of the frame host forms, for npx pixels: linear [npx][3] doubles and rgb8 [npx][3] bytes always; stderr [npx] doubles, the two metrics
// counters and samples [npx] ints where wanted (else null).  Each comes back to the host array the caller gave for it.  (A progressive frame keeps
// its counters in its own buffer: those forms want no plane and copy from there.)
struct FramePlanes {
    double *lin = nullptr, *err = nullptr;
    u64 *cnt = nullptr;
    int *smp = nullptr;
    unsigned char *q = nullptr;
    int reserve(HostIo &io, size_t npx, bool want_err, bool want_cnt, bool want_smp, double *out_linear, uint8_t *out_rgb8, double *out_stderr,
                int32_t *out_samples, uint64_t *out_counters) {
        io.work(&lin, npx * 3, out_linear); io.plane(&err, npx, want_err, nullptr, out_stderr); io.plane(&cnt, 2, want_cnt, nullptr, out_counters);
        io.plane(&smp, npx, want_smp, nullptr, out_samples); io.work(&q, npx * 3, out_rgb8);
        return io.reserve();
    }
};

} // namespace

// ---- library / context -------------------------------------------------------------------------------
// test hook, host code only (no device): the device's tree (+ entry grid) over n spheres as rtmi_scene_create builds it, on the team or (threads = 1) on the
// calling thread alone.  out_hash = FNV-1a of the node array and the grid's root codes, out_info = {node records, depth, grid cells per side, big primitives}
RTMI_EXPORT int rtmi_test_build_tree(int32_t n, const double *geom, const double *cam, int32_t threads, uint64_t *out_hash, int32_t *out_info, double *out_ms) {
    if (n <= 0 || !geom || !cam || !out_hash || !out_info || !out_ms) return fail(RTMI_E_ARG, "bad arguments");
    const BuildKnobs knobs = read_build_knobs();
    std::vector<int> kind((size_t)n, RTMI_PRIM_SPHERE);
    std::vector<BvhBox> wbox((size_t)n);
    std::vector<char> bounded((size_t)n, 0), box_first((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        const double g[9] = {geom[4 * (size_t)i], geom[4 * (size_t)i + 1], geom[4 * (size_t)i + 2], geom[4 * (size_t)i + 3], 0, 0, 0, 0, 1};
        bounded[(size_t)i] = prim_world_box(RTMI_PRIM_SPHERE, g, nullptr, nullptr, 0, 0, 0.0, 1.0, wbox[(size_t)i]);
    }
    DevScene d{};
    std::vector<int> grid_cells;
    int depth = 0;
    g_build_single.store(threads == 1 ? 1 : 0);
    const double t0 = now_ms();
    const std::vector<float> nodes = build_bvh(d, n, kind.data(), wbox, bounded, cam, true, grid_cells, box_first, knobs, &depth);
    *out_ms = now_ms() - t0;
    g_build_single.store(0);
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void *p, size_t bytes) { const unsigned char *q = (const unsigned char *)p; for (size_t k = 0; k < bytes; ++k) { h ^= q[k]; h *= 1099511628211ull; } };
    mix(nodes.data(), nodes.size() * sizeof(float));
    mix(grid_cells.data(), grid_cells.size() * sizeof(int));
    mix(&d.bvh_root, sizeof(int)); mix(&d.grid_tall, sizeof(int)); mix(&d.bvh_node16, sizeof(int));
    *out_hash = h;
    out_info[0] = (int32_t)(nodes.size() / (d.bvh_node16 ? 8 : 16)); out_info[1] = depth; out_info[2] = d.grid_n; out_info[3] = d.n_big;
    return RTMI_OK;
}
RTMI_EXPORT int rtmi_test_camera_fixed(int32_t cam_kind, const double *cam) { // test hook (host arithmetic only: no device needed)
    const int o = camera_fixed_origin(cam_kind, cam);
    return o | (camera_fixed_rays(cam_kind, o, cam) << 1);
}
RTMI_EXPORT int rtmi_test_half_outward(double x, int32_t up) { return (int)half_outward((float)x, up != 0); } // test hook (host arithmetic only: no device needed)
// test hook, host code only (no device): where HostIo puts n planes of elem_bytes[i] * counts[i] bytes (present[i] = 0: the caller left the plane out).
// out_offsets[i] = the plane's first byte in the arena (UINT64_MAX for an absent plane), out_total = the bytes the arena needs
RTMI_EXPORT int rtmi_test_stage_layout(int32_t n, const uint64_t *elem_bytes, const uint64_t *counts, const int32_t *present, uint64_t *out_offsets, uint64_t *out_total) {
    if (n < 0 || (n && (!elem_bytes || !counts || !present || !out_offsets)) || !out_total) return fail(RTMI_E_ARG, "bad arguments");
    std::vector<IoPlane> pl((size_t)n);
    for (int i = 0; i < n; ++i) pl[(size_t)i] = {(size_t)elem_bytes[i], (size_t)counts[i], present[i] != 0, nullptr, nullptr, nullptr, 0};
    *out_total = io_layout(pl.data(), n);
    for (int i = 0; i < n; ++i) out_offsets[i] = pl[(size_t)i].present ? pl[(size_t)i].off : UINT64_MAX;
    return RTMI_OK;
}
RTMI_EXPORT const char *rtmi_last_error(void) { return g_err.c_str(); }
RTMI_EXPORT const char *rtmi_backend_name(void) { return "hip-gfx950"; }
RTMI_EXPORT int rtmi_version(void) { return 220; } // 220: light-sampled frames on several GPUs (rtmi_lit_tiles_records_device, rtmi_multi_lit_*); 219: light-sampled frames over a caller's tile list and the stateless retirement (rtmi_render_lit_tiles*, rtmi_tiles_retire*); 218: direct lighting from the scene's area lights (rtmi_scene_lights, rtmi_direct_irradiance*, rtmi_render_direct*); 217: occlusion rays generated on the device (rtmi_occlusion_hemisphere*, rtmi_occlusion_targets*, rtmi_ambient_occlusion*); 216: closest-hit and any-hit queries (rtmi_query_hits*, rtmi_query_occluded*); 215: caller-supplied rays (rtmi_render_rays*); 214: the geometry of a live scene (rtmi_scene_set_geometry: the trees refit on the device); 213: the materials of a live scene (rtmi_scene_set_materials, rtmi_scene_set_materials_stream); 212: rtmi_scene_tree_info; 211: rtmi_reproject* (temporal accumulation); 210: the camera of a live scene (rtmi_scene_set_camera, rtmi_scene_set_camera_stream, rtmi_scene_camera); 209: progressive / adaptive frames on dealt tiles and several devices (rtmi_render_adaptive_tiles_device, rtmi_assemble_progressive_device, rtmi_render_multi_adaptive*); 208: tiles retired by a caller's noise map (rtmi_adaptive_retire*); 207: first-hit feature buffers and the edge-aware denoiser (rtmi_render_features*, rtmi_denoise*); 206: adaptive sampling (rtmi_render_adaptive*, rtmi_adaptive_status, rtmi_adaptive_active_tiles); 205: progressive rendering (rtmi_render_progressive*, rtmi_progressive_samples / _release); 204: rtmi_probe_math2
RTMI_EXPORT uint64_t rtmi_sample_key(uint64_t seed, uint64_t pixel, uint64_t sample) { return sample_key(seed, pixel, sample); }

RTMI_EXPORT int rtmi_init(int device, uint32_t flags, rtmi_ctx **out_ctx) {
    if (!out_ctx) return fail(RTMI_E_ARG, "out_ctx is NULL");
    *out_ctx = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(RTMI_E_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(RTMI_E_ARG, "device %d out of range (0..%d)", device, ndev - 1);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RTMI_E_DEVICE, "device %d is %s; this library carries gfx950 (MI355X) code objects only", device, prop.gcnArchName);
    rtmi_ctx *c = new (std::nothrow) rtmi_ctx();
    if (!c) return fail(RTMI_E_NOMEM, "out of host memory");
    c->device = device;
    c->flags = flags;
    c->cus = prop.multiProcessorCount;
    c->lds_per_cu = (int)prop.maxSharedMemoryPerMultiProcessor;
    c->hbm = prop.totalGlobalMem;
    c->arch = prop.gcnArchName;
    if (const char *e = std::getenv("RTMI_BLOCKS_PER_CU")) c->blocks_per_cu = std::max(1, std::atoi(e));
    if (const char *e = std::getenv("RTMI_SCAN_VARIANT")) c->scan_variant = std::min(3, std::max(0, std::atoi(e)));
    if (const char *e = std::getenv("RTMI_LDS_TILE_BYTES")) c->max_lds_bytes = std::min(64 * 1024 - 64, std::max(1024, std::atoi(e)));
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return fail(RTMI_E_DEVICE, "hipStreamCreate failed"); }
    *out_ctx = c;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_shutdown(rtmi_ctx *c) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
#ifdef RTMI_HIST
    { unsigned long long h[200]; if (hipMemcpyFromSymbol(h, HIP_SYMBOL(rtmi::g_hist), sizeof h) == hipSuccess) { for (int k = 0; k < 3; ++k) { fprintf(stderr, "HIST%d", k); for (int i = 0; i <= 64; ++i) fprintf(stderr, " %llu", h[64 * k + i]); fprintf(stderr, "\n"); } } }
#endif
    c->samples.release(); c->accum.release(); c->tiles.release(); c->tile_ids.release(); c->counters.release(); c->io.release(); c->multi.release();
    c->prog.release();
    c->feat_cnt.release(); c->dn_planes.release(); c->rays_ws.release(); c->occ_ws.release(); c->direct_ws.release(); c->nee_ws.release(); c->retire_ws.release();
    for (hipEvent_t e : {c->ev_done, c->ev_g0, c->ev_g1}) if (e) (void)hipEventDestroy(e);
    if (c->ev_consumed) { (void)hipSetDevice(c->ev_consumed_device); (void)hipEventDestroy(c->ev_consumed); (void)hipSetDevice(c->device); }
    for (auto &e : c->events) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (hipEvent_t e : c->events_r) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c->stream);
    c->magic = 0;
    delete c;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_set_option(rtmi_ctx *c, const char *name, int64_t value) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (!name) return fail(RTMI_E_ARG, "name is NULL");
    if (!std::strcmp(name, "blocks_per_cu")) { if (value < 1 || value > 64) return fail(RTMI_E_ARG, "blocks_per_cu must be 1..64"); c->blocks_per_cu = (int)value; return RTMI_OK; }
    if (!std::strcmp(name, "workspace_bytes")) { if (value < (1 << 20)) return fail(RTMI_E_ARG, "workspace_bytes must be >= 1 MiB"); c->workspace_bytes = value; return RTMI_OK; }
    if (!std::strcmp(name, "lds_tile_bytes")) { if (value < 1024 || value > 64 * 1024 - 64) return fail(RTMI_E_ARG, "lds_tile_bytes out of range"); c->max_lds_bytes = (int)value; return RTMI_OK; }
    if (!std::strcmp(name, "timing")) { if (value) c->flags |= RTMI_FLAG_TIMING; else c->flags &= ~RTMI_FLAG_TIMING; return RTMI_OK; }
    if (!std::strcmp(name, "scan_variant")) { if (value < 0 || value > 3) return fail(RTMI_E_ARG, "scan_variant must be 0..3"); c->scan_variant = (int)value; return RTMI_OK; }
    if (!std::strcmp(name, "count_traversal")) { c->count_traversal = value ? 1 : 0; return RTMI_OK; }
    if (!std::strcmp(name, "defer_emitters")) { if (value < 0 || value > 1) return fail(RTMI_E_ARG, "defer_emitters must be 0 or 1"); c->defer_emitters = (int)value; return RTMI_OK; }
    if (!std::strcmp(name, "test_fail_next_render")) { c->fail_next_render = value ? 1 : 0; return RTMI_OK; }
    if (!std::strcmp(name, "test_fail_allocs")) { c->fail_allocs = (int)std::max<int64_t>(0, std::min<int64_t>(value, 64)); return RTMI_OK; }
    if (!std::strcmp(name, "flat_below")) { if (value < 0 || value > (1 << 20)) return fail(RTMI_E_ARG, "flat_below must be 0..2^20"); c->flat_below = (int)value; return RTMI_OK; }
    if (!std::strcmp(name, "suspend_lanes")) { if (value < 0 || value > 64) return fail(RTMI_E_ARG, "suspend_lanes must be 0..64"); c->suspend_lanes = (int)value; c->suspend_lanes_set = true; return RTMI_OK; }
    if (!std::strcmp(name, "accel")) {
        if (value == RTMI_ACCEL_FLAT || value == RTMI_ACCEL_BVH) { c->accel = (int)value; return RTMI_OK; }
        return fail(RTMI_E_UNSUPPORTED, "accel %lld is not available in this build", (long long)value);
    }
    return fail(RTMI_E_ARG, "unknown option '%s'", name);
}

RTMI_EXPORT int rtmi_device_info(rtmi_ctx *c, int32_t *cus, int32_t *lds, int64_t *hbm, char *arch, int32_t arch_len) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (cus) *cus = c->cus;
    if (lds) *lds = c->lds_per_cu;
    if (hbm) *hbm = (int64_t)c->hbm;
    if (arch && arch_len > 0) { std::strncpy(arch, c->arch.c_str(), (size_t)arch_len - 1); arch[arch_len - 1] = 0; }
    return RTMI_OK;
}

// ---- scene ---------------------------------------------------------------------------------------------
RTMI_EXPORT int rtmi_scene_create(rtmi_ctx *c, int32_t n_prims, const int32_t *prim_kind, const double *prim_geom, const int32_t *prim_mat,
                                  int32_t n_mats, const int32_t *mat_kind, const int32_t *mat_tex, const double *mat_param,
                                  int32_t n_tex, const int32_t *tex_kind, const double *tex_param, const int32_t *tex_child,
                                  int32_t cam_kind, const double *cam, rtmi_scene **out_scene) {
    return rtmi_scene_create_ex(c, n_prims, prim_kind, prim_geom, prim_mat, n_mats, mat_kind, mat_tex, mat_param, n_tex, tex_kind, tex_param, tex_child,
                                cam_kind, cam, nullptr, nullptr, 0, nullptr, nullptr, out_scene);
}

// DevScene::media_fast follows the media call sequence
static void fill_media_fast(DevScene &d, const std::map<int, std::array<double, 5>> &media_fast_of) {
    for (int k = 0; k < 8; ++k) {
        double *q = d.media_fast[k];
        for (int j = 0; j < 8; ++j) q[j] = 0.0;
        if (k >= d.n_media) continue;
        const auto it = media_fast_of.find(d.media_idx[k]);
        if (it == media_fast_of.end()) continue;
        q[0] = 1.0;
        for (int j = 0; j < 5; ++j) q[1 + j] = it->second[(size_t)j];
    }
}
static void fill_media_fast(rtmi_scene *s) { fill_media_fast(s->dev, s->media_fast_of); }
namespace {
// The checks of the material and texture tables, shared by rtmi_scene_create_ex and rtmi_scene_set_materials*: the kind ranges, the texture and child indices, the
// image indices.  This is where "unknown record type -> explicit unsupported error" surfaces
int check_material_tables(const SceneArrays &a) {
    const int n_mats = a.n_mats, n_tex = a.n_tex;
    const int32_t *mat_kind = a.mat_kind, *mat_tex = a.mat_tex, *tex_kind = a.tex_kind, *tex_child = a.tex_child;
    for (int t = 0; t < n_tex; ++t) {
        if (tex_kind[t] < RTMI_TEX_CONSTANT || tex_kind[t] > RTMI_TEX_IMAGE) return fail(RTMI_E_UNSUPPORTED, "texture %d: kind %d unsupported on GPU path", t, tex_kind[t]);
        if (tex_kind[t] == RTMI_TEX_FLIP_U || tex_kind[t] == RTMI_TEX_FLIP_V) {
            const int ch = tex_child[2 * t];
            if (ch < 0 || ch >= n_tex || ch == t) return fail(RTMI_E_ARG, "texture %d: wrapped texture %d invalid", t, ch);
        }
        if (tex_kind[t] == RTMI_TEX_CHECKER)
            for (int k = 0; k < 2; ++k) {
                const int ch = tex_child[2 * t + k];
                if (ch < 0 || ch >= n_tex || ch == t) return fail(RTMI_E_ARG, "texture %d: checker child %d invalid", t, ch);
            }
    }
    for (int m = 0; m < n_mats; ++m) {
        if (mat_kind[m] < RTMI_MAT_LAMBERTIAN || mat_kind[m] > RTMI_MAT_ISOTROPIC) return fail(RTMI_E_UNSUPPORTED, "material %d: kind %d unsupported on GPU path", m, mat_kind[m]);
        if (mat_kind[m] != RTMI_MAT_DIELECTRIC && (mat_tex[m] < 0 || mat_tex[m] >= n_tex)) return fail(RTMI_E_ARG, "material %d: texture index %d invalid", m, mat_tex[m]);
    }
    for (int t = 0; t < n_tex; ++t)
        if (tex_kind[t] == RTMI_TEX_IMAGE) {
            const double im = a.tex_param[(size_t)t * RTMI_TEX_STRIDE];
            if (!(im >= 0 && im < 1e6 && im == std::floor(im))) return fail(RTMI_E_ARG, "texture %d: image index invalid", t);
        }
    return RTMI_OK;
}
// ... and of primitive i's material: its index, and (after the index: it reads the material) the phase function of a medium
int check_prim_material(const SceneArrays &a, int i) {
    if (a.prim_mat[i] < 0 || a.prim_mat[i] >= a.n_mats) return fail(RTMI_E_ARG, "primitive %d: material index %d invalid", i, a.prim_mat[i]);
    return RTMI_OK;
}
int check_medium_material(const SceneArrays &a, int i) {
    if (a.mat_kind[a.prim_mat[i]] != RTMI_MAT_ISOTROPIC) return fail(RTMI_E_ARG, "medium %d: the phase function must be RTMI_MAT_ISOTROPIC", i);
    return RTMI_OK;
}
// the checks of rtmi_scene_create_ex, in the order they are reported
int check_scene_args(const SceneArrays &a, rtmi_scene **out_scene) {
    const int n_prims = a.n_prims, n_mats = a.n_mats, n_tex = a.n_tex, n_xforms = a.n_xforms;
    const int32_t *prim_kind = a.prim_kind, *prim_mat = a.prim_mat, *mat_kind = a.mat_kind, *mat_tex = a.mat_tex, *tex_kind = a.tex_kind, *tex_child = a.tex_child;
    if (n_xforms < 0 || (n_xforms > 0 && (!a.xform_kind || !a.xform_param || !a.prim_xform))) return fail(RTMI_E_ARG, "xform arrays are NULL");
    for (int k = 0; k < n_xforms; ++k)
        if (a.xform_kind[k] != RTMI_XFORM_TRANSLATE && a.xform_kind[k] != RTMI_XFORM_ROTATE_Y) return fail(RTMI_E_UNSUPPORTED, "xform %d: kind %d unsupported on GPU path", k, a.xform_kind[k]);
    if (!out_scene) return fail(RTMI_E_ARG, "out_scene is NULL");
    *out_scene = nullptr;
    if (n_prims < 0 || n_mats < 0 || n_tex < 0) return fail(RTMI_E_ARG, "negative count");
    if (n_prims > 0 && (!prim_kind || !a.prim_geom || !prim_mat)) return fail(RTMI_E_ARG, "primitive arrays are NULL");
    if (n_mats > 0 && (!mat_kind || !mat_tex || !a.mat_param)) return fail(RTMI_E_ARG, "material arrays are NULL");
    if (n_tex > 0 && (!tex_kind || !a.tex_param || !tex_child)) return fail(RTMI_E_ARG, "texture arrays are NULL");
    if (!a.cam) return fail(RTMI_E_ARG, "cam is NULL");
    if (a.cam_kind != RTMI_CAM_PINHOLE && a.cam_kind != RTMI_CAM_THINLENS) return fail(RTMI_E_UNSUPPORTED, "camera kind %d unsupported on GPU path", a.cam_kind);
    int rc = check_material_tables(a);
    if (rc) return rc;
    int n_world = 0, n_media = 0;
    for (int i = 0; i < n_prims; ++i) {
        const int kind = prim_kind[i] & ~RTMI_PRIM_BOUNDARY;
        const bool is_boundary = (prim_kind[i] & RTMI_PRIM_BOUNDARY) != 0;
        if (kind < RTMI_PRIM_SPHERE || kind > RTMI_PRIM_MEDIUM) return fail(RTMI_E_UNSUPPORTED, "primitive %d: kind %d unsupported on GPU path", i, prim_kind[i]);
        if (is_boundary && kind == RTMI_PRIM_MEDIUM) return fail(RTMI_E_UNSUPPORTED, "primitive %d: a medium inside a medium's boundary is unsupported", i);
        if (!is_boundary && n_world != i) return fail(RTMI_E_ARG, "primitive %d: boundary primitives must come after all world primitives", i);
        if (!is_boundary) n_world = i + 1;
        if ((rc = check_prim_material(a, i)) != RTMI_OK) return rc;
        if (kind == RTMI_PRIM_MEDIUM) {
            const double *mg = a.prim_geom + (size_t)i * RTMI_PRIM_STRIDE;
            const int fb = (int)mg[1], nb = (int)mg[2];
            if (!(mg[0] == mg[0]) || fb < 0 || nb <= 0 || fb + nb > n_prims) return fail(RTMI_E_ARG, "medium %d: boundary range [%d, %d) invalid", i, fb, fb + nb);
            for (int q = fb; q < fb + nb; ++q) if (!(prim_kind[q] & RTMI_PRIM_BOUNDARY)) return fail(RTMI_E_ARG, "medium %d: primitive %d is not flagged RTMI_PRIM_BOUNDARY", i, q);
            if ((rc = check_medium_material(a, i)) != RTMI_OK) return rc;
            if (n_media++ >= 16) return fail(RTMI_E_UNSUPPORTED, "more than 16 ConstantMedium records in one scene");
            continue;
        }
        if (is_boundary) continue;
        const int xf_first = a.prim_xform ? a.prim_xform[2 * i] : 0, xf_count = a.prim_xform ? a.prim_xform[2 * i + 1] : 0;
        if (xf_count < 0 || xf_first < 0 || xf_first + xf_count > n_xforms) return fail(RTMI_E_ARG, "primitive %d: xform range [%d, %d) invalid", i, xf_first, xf_first + xf_count);
    }
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_scene_create_ex(rtmi_ctx *c, int32_t n_prims, const int32_t *prim_kind, const double *prim_geom, const int32_t *prim_mat,
                                     int32_t n_mats, const int32_t *mat_kind, const int32_t *mat_tex, const double *mat_param,
                                     int32_t n_tex, const int32_t *tex_kind, const double *tex_param, const int32_t *tex_child,
                                     int32_t cam_kind, const double *cam, const int32_t *prim_flip, const int32_t *prim_xform,
                                     int32_t n_xforms, const int32_t *xform_kind, const double *xform_param, rtmi_scene **out_scene) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    const double t_create0 = now_ms();
    const SceneArrays a{n_prims, prim_kind, prim_geom, prim_mat, n_mats, mat_kind, mat_tex, mat_param, n_tex, tex_kind, tex_param, tex_child,
                        cam_kind, cam, prim_flip, prim_xform, n_xforms, xform_kind, xform_param};
    int rc = check_scene_args(a, out_scene);
    if (rc) return rc;
    const BuildKnobs knobs = read_build_knobs();
    HIP_TRY(hipSetDevice(c->device));
    rtmi_scene *s = new (std::nothrow) rtmi_scene();
    if (!s) return fail(RTMI_E_NOMEM, "out of host memory");
    PackedScene P = pack_scene(a, knobs);
    s->ctx = c; s->n_prims = n_prims; s->n_mats = n_mats; s->n_tex = n_tex;
    s->serial = ++g_scene_serial;
    s->uses_perlin = P.M.uses_perlin; s->max_image = P.M.max_image; s->bvh_node_count = P.bvh_node_count; s->bvh_depth = P.bvh_depth;
    s->host_kind = P.host_kind; s->media_fast_of = P.media_fast_of; s->dev = P.d; s->geom_ext = P.geom_ext; s->tree = std::move(P.tree);
    for (int k : s->host_kind) s->has_moving = s->has_moving || k == RTMI_PRIM_MOVING;
    DevScene &d = s->dev;
    rc = upload_tables(P, d, s->table_allocs, s->table_bytes);
    s->device_bytes += s->table_bytes;
    s->mat = std::move(P.M); // (uploaded: the scene keeps the host copy)
    fill_media_fast(s);
    if (!rc) {
        std::vector<DevScene> one(1, d);
        const DevScene *dp = nullptr;
        rc = upload(s, Table(one, &dp));
        s->d_dev = (ScenePtr)dp;
    }
    if (rc) { rtmi_scene_destroy(s); return rc; }
    if (knobs.debug)
        fprintf(stderr, "[rtmi] scene create: records %.2f ms, trees %.2f ms, tables + upload (%zu allocations, %.2f MB) %.2f ms\n", P.t_tree0 - t_create0, P.t_tree1 - P.t_tree0,
                s->allocs.size() + s->table_allocs.size(), (double)s->device_bytes / 1e6, now_ms() - P.t_tree1);
    {
        rtmi_scene::Args &A = s->args;
        A.prim_kind.assign(prim_kind, prim_kind + n_prims); A.prim_mat.assign(prim_mat, prim_mat + n_prims);
        A.prim_geom.assign(prim_geom, prim_geom + (size_t)n_prims * RTMI_PRIM_STRIDE);
        A.mat_kind.assign(mat_kind, mat_kind + n_mats); A.mat_tex.assign(mat_tex, mat_tex + n_mats); A.mat_param.assign(mat_param, mat_param + n_mats);
        A.tex_kind.assign(tex_kind, tex_kind + n_tex); A.tex_param.assign(tex_param, tex_param + (size_t)n_tex * RTMI_TEX_STRIDE);
        A.tex_child.assign(tex_child, tex_child + 2 * (size_t)n_tex);
        A.cam.assign(cam, cam + 24); A.cam_kind = cam_kind;
        if (prim_flip) A.prim_flip.assign(prim_flip, prim_flip + n_prims);
        if (prim_xform) A.prim_xform.assign(prim_xform, prim_xform + 2 * (size_t)n_prims);
        if (n_xforms > 0) { A.xform_kind.assign(xform_kind, xform_kind + n_xforms); A.xform_param.assign(xform_param, xform_param + 3 * (size_t)n_xforms); }
    }
    *out_scene = s;
    return RTMI_OK;
}

namespace {
int reupload_descriptor(rtmi_scene *s) {
    fill_media_fast(s);
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    HIP_TRY(hipMemcpy((void *)s->d_dev, &s->dev, sizeof(DevScene), hipMemcpyHostToDevice));
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_scene_set_perlin(rtmi_scene *s, const double *vectors, const int32_t *perm) {
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    if (!vectors || !perm) return fail(RTMI_E_ARG, "NULL array");
    for (int a = 0; a < 3; ++a) { // each must be a permutation of 0..255 (perlin.clj:10-17)
        bool seen[256] = {false};
        for (int k = 0; k < 256; ++k) {
            const int v = perm[a * 256 + k];
            if (v < 0 || v > 255 || seen[v]) return fail(RTMI_E_ARG, "perm-%c is not a permutation of 0..255", "xyz"[a]);
            seen[v] = true;
        }
    }
    HIP_TRY(hipSetDevice(s->ctx->device));
    s->revision++;
    std::vector<double> v(vectors, vectors + 768);
    std::vector<int> p(perm, perm + 768);
    int rc = upload(s, Table(v, &s->dev.perlin_vec));
    if (!rc) rc = upload(s, Table(p, &s->dev.perlin_perm));
    if (rc) return rc;
    s->have_perlin = true;
    s->args.perlin_vec = v; s->args.perm.assign(perm, perm + 768);
    return reupload_descriptor(s);
}

RTMI_EXPORT int rtmi_scene_set_media_calls(rtmi_scene *s, int32_t n_calls, const int32_t *calls) {
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    if (n_calls < 0 || n_calls > 32 || (n_calls > 0 && !calls)) return fail(RTMI_E_ARG, "n_calls must be 0..32");
    for (int k = 0; k < n_calls; ++k)
        if (calls[k] < 0 || calls[k] >= s->n_prims || s->host_kind[(size_t)calls[k]] != RTMI_PRIM_MEDIUM) return fail(RTMI_E_ARG, "calls[%d] = %d is not a medium primitive", k, calls[k]);
    if (s->dev.media_seq == 1)
        for (int k = 1; k < n_calls; ++k) if (calls[k] <= calls[k - 1]) return fail(RTMI_E_ARG, "RTMI_MEDIA_HITLIST: the media must be called once each, in ascending primitive (= list) order");
    s->revision++;
    if (s->dev.media_seq == 2) { s->dev.media_seq = 0; s->args.media_mode = 0; } // a plain call sequence replaces a narrowed one
    s->dev.n_media = n_calls;
    for (int k = 0; k < n_calls; ++k) { s->dev.media_idx[k] = calls[k]; s->dev.media_lo[k] = calls[k]; }
    s->args.media_calls.assign(calls, calls + n_calls); s->args.has_media_calls = true;
    HIP_TRY(hipSetDevice(s->ctx->device));
    return reupload_descriptor(s);
}

// RTMI_MEDIA_NARROWED: the media call sequence with, per call, the first primitive of the Hitlist items that narrow its t-max (narrow_from[k] = calls[k]: none)
RTMI_EXPORT int rtmi_scene_set_media_calls_narrowed(rtmi_scene *s, int32_t n_calls, const int32_t *calls, const int32_t *narrow_from) {
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    if (n_calls < 0 || n_calls > 32 || (n_calls > 0 && (!calls || !narrow_from))) return fail(RTMI_E_ARG, "n_calls must be 0..32");
    for (int k = 0; k < n_calls; ++k) {
        if (calls[k] < 0 || calls[k] >= s->n_prims || s->host_kind[(size_t)calls[k]] != RTMI_PRIM_MEDIUM) return fail(RTMI_E_ARG, "calls[%d] = %d is not a medium primitive", k, calls[k]);
        if (narrow_from[k] < 0 || narrow_from[k] > calls[k]) return fail(RTMI_E_ARG, "narrow_from[%d] = %d must lie in [0, calls[%d] = %d]", k, narrow_from[k], k, calls[k]);
        if (k > 0 && narrow_from[k] < calls[k] && narrow_from[k] == narrow_from[k - 1] && calls[k] <= calls[k - 1])
            return fail(RTMI_E_ARG, "calls %d and %d share a narrowing Hitlist and must come in list order", k - 1, k);
    }
    s->revision++;
    s->dev.n_media = n_calls;
    bool any = false;
    for (int k = 0; k < n_calls; ++k) { s->dev.media_idx[k] = calls[k]; s->dev.media_lo[k] = narrow_from[k]; any = any || narrow_from[k] < calls[k]; }
    s->dev.media_seq = any ? 2 : 0;
    s->args.media_calls.assign(calls, calls + n_calls); s->args.media_lo.assign(narrow_from, narrow_from + n_calls); s->args.has_media_calls = true;
    s->args.media_mode = any ? 2 : 0;
    HIP_TRY(hipSetDevice(s->ctx->device));
    return reupload_descriptor(s);
}

RTMI_EXPORT int rtmi_scene_set_media_mode(rtmi_scene *s, int32_t mode) {
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    if (mode != RTMI_MEDIA_DESCENT && mode != RTMI_MEDIA_HITLIST) return fail(RTMI_E_ARG, "mode must be RTMI_MEDIA_DESCENT or RTMI_MEDIA_HITLIST");
    if (mode == RTMI_MEDIA_HITLIST)
        for (int k = 1; k < s->dev.n_media; ++k)
            if (s->dev.media_idx[k] <= s->dev.media_idx[k - 1]) return fail(RTMI_E_ARG, "RTMI_MEDIA_HITLIST: the media must be called once each, in ascending primitive (= list) order");
    s->revision++;
    s->dev.media_seq = mode == RTMI_MEDIA_HITLIST ? 1 : 0;
    s->args.media_mode = mode;
    HIP_TRY(hipSetDevice(s->ctx->device));
    return reupload_descriptor(s);
}

RTMI_EXPORT int rtmi_scene_set_images(rtmi_scene *s, int32_t n_images, const int32_t *wh, const uint8_t *rgb) {
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    if (n_images < 0 || (n_images > 0 && (!wh || !rgb))) return fail(RTMI_E_ARG, "bad image arguments");
    std::vector<int> whv;
    std::vector<long long> off;
    long long total = 0;
    for (int i = 0; i < n_images; ++i) {
        if (wh[2 * i] <= 0 || wh[2 * i + 1] <= 0 || wh[2 * i] > 65536 || wh[2 * i + 1] > 65536) return fail(RTMI_E_ARG, "image %d: bad size %dx%d", i, wh[2 * i], wh[2 * i + 1]);
        whv.push_back(wh[2 * i]); whv.push_back(wh[2 * i + 1]);
        off.push_back(total);
        total += (long long)wh[2 * i] * wh[2 * i + 1] * 3;
    }
    HIP_TRY(hipSetDevice(s->ctx->device));
    s->revision++;
    std::vector<unsigned char> px(rgb, rgb + total);
    int rc = upload(s, Table(whv, &s->dev.image_wh));
    if (!rc) rc = upload(s, Table(off, &s->dev.image_off));
    if (!rc) rc = upload(s, Table(px, &s->dev.image_rgb));
    if (rc) return rc;
    s->dev.n_images = n_images;
    s->args.image_wh = whv; s->args.image_rgb = px;
    return reupload_descriptor(s);
}

// ---- the camera of a live scene (rtmi_scene_set_camera*) ---------------------------------------------------------------------------------------
namespace {
// What a camera move changes in the descriptor: the last three fields of DevScene, one contiguous range
constexpr size_t kCamOffset = offsetof(DevScene, cam_kind), kCamBytes = sizeof(DevScene) - offsetof(DevScene, cam_kind);
static_assert(offsetof(DevScene, cam_fixed_origin) == offsetof(DevScene, cam_kind) + sizeof(int) && offsetof(DevScene, cam) == offsetof(DevScene, cam_kind) + 2 * sizeof(int) &&
              kCamBytes == 2 * sizeof(int) + 24 * sizeof(double), "cam_kind, cam_fixed_origin and cam[24] end the descriptor");
struct CameraArgs { double cam[24]; int cam_kind, cam_fixed_origin; };

// One wave, in stream order: lane l < 24 stores cam[l], lanes 24 and 25 the two ints.  Plain vector stores; the renders queued behind it on the stream read the
// descriptor through the scalar cache, which every kernel launch invalidates.  No LDS, no scratch.
__global__ void __launch_bounds__(64) set_camera_kernel(DevScene *d, CameraArgs a) {
    const int l = (int)threadIdx.x;
    if (l < 24) d->cam[l] = a.cam[l];
    else if (l == 24) d->cam_kind = a.cam_kind;
    else if (l == 25) d->cam_fixed_origin = a.cam_fixed_origin;
}

// the argument errors of both set forms, reported before the handle is examined
int check_camera_args(int cam_kind, const double *cam) {
    if (!cam) return fail(RTMI_E_ARG, "cam is NULL");
    if (cam_kind != RTMI_CAM_PINHOLE && cam_kind != RTMI_CAM_THINLENS) return fail(RTMI_E_UNSUPPORTED, "camera kind %d unsupported on GPU path", cam_kind);
    return RTMI_OK;
}
// The camera FITS the built scene: no MovingSphere, or its shutter interval lies inside the interval the swept bounds were built for
bool camera_fits(const rtmi_scene *s, int cam_kind, const double *cam, double *t_lo, double *t_hi) {
    camera_shutter(cam_kind, cam, *t_lo, *t_hi);
    return !s->has_moving || (*t_lo >= s->dev.cull_t_lo && *t_hi <= s->dev.cull_t_hi);
}
// the host's half of a camera move: the mirror of the descriptor (launch decisions read it) and the arguments a clone replays
void adopt_camera(rtmi_scene *s, int cam_kind, const double *cam) {
    s->dev.cam_kind = cam_kind;
    std::memcpy(s->dev.cam, cam, 24 * sizeof(double));
    s->dev.cam_fixed_origin = camera_fixed_origin(cam_kind, cam);
    s->args.cam.assign(cam, cam + 24); s->args.cam_kind = cam_kind;
    s->revision++;
}
// The arrays the scene keeps, as pack_scene takes them: what a rebuild starts from.  The callers replace the camera, or the materials, by their own.
SceneArrays kept_arrays(const rtmi_scene *s) {
    const rtmi_scene::Args &A = s->args;
    return SceneArrays{s->n_prims, A.prim_kind.data(), A.prim_geom.data(), A.prim_mat.data(), s->n_mats, A.mat_kind.data(), A.mat_tex.data(), A.mat_param.data(),
                       s->n_tex, A.tex_kind.data(), A.tex_param.data(), A.tex_child.data(), A.cam_kind, A.cam.data(),
                       A.prim_flip.empty() ? nullptr : A.prim_flip.data(), A.prim_xform.empty() ? nullptr : A.prim_xform.data(),
                       (int)A.xform_kind.size(), A.xform_kind.empty() ? nullptr : A.xform_kind.data(), A.xform_param.empty() ? nullptr : A.xform_param.data()};
}
// The slow path of a camera or material edit: the staged build from `a` (the arrays the scene keeps, with the edited ones in their place), new tables uploaded
// beside the old ones, then the swap.  Until the swap nothing of the scene has changed; a failure frees what was uploaded and leaves it as it was.  The caller
// adopts the edited arrays into rtmi_scene::Args afterwards (`a` may point into them) and bumps the revision.
void drop_geometry_edit(rtmi_scene *s) {
    if (s->geo.d_order) (void)hipFree(s->geo.d_order);
    if (s->geo.d_leaf_box) (void)hipFree(s->geo.d_leaf_box);
    if (s->geo.ev0) (void)hipEventDestroy(s->geo.ev0);
    if (s->geo.ev1) (void)hipEventDestroy(s->geo.ev1);
    s->device_bytes -= s->geo.bytes;
    s->geo = rtmi_scene::GeoEdit();
}
int rebuild_scene(rtmi_scene *s, const SceneArrays &a, const char *what) {
    PackedScene P = pack_scene(a, read_build_knobs());
    DevScene nd = P.d;
    std::vector<void *> fresh;
    size_t fresh_bytes = 0;
    int rc = upload_tables(P, nd, fresh, fresh_bytes);
    if (!rc) {
        // what the rtmi_scene_set_* calls gave the scene (kept in Args for the clones) stays: the Perlin tables and the images where they are in HBM, the media
        // call sequence -- a narrowed one too -- and the media mode as the descriptor holds them
        const DevScene &o = s->dev;
        nd.perlin_vec = o.perlin_vec; nd.perlin_perm = o.perlin_perm;
        nd.n_images = o.n_images; nd.image_wh = o.image_wh; nd.image_off = o.image_off; nd.image_rgb = o.image_rgb;
        nd.n_media = o.n_media; nd.media_seq = o.media_seq;
        std::memcpy(nd.media_idx, o.media_idx, sizeof nd.media_idx); std::memcpy(nd.media_lo, o.media_lo, sizeof nd.media_lo);
        fill_media_fast(nd, P.media_fast_of);
        hipError_t e = hipStreamSynchronize(s->ctx->stream); // the renders in flight read the old tables
        if (e == hipSuccess) e = hipMemcpy((void *)s->d_dev, &nd, sizeof(DevScene), hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail(RTMI_E_DEVICE, "%s: %s", what, hipGetErrorString(e));
    }
    if (rc) { for (void *p : fresh) (void)hipFree(p); return rc; }
    for (void *p : s->table_allocs) (void)hipFree(p); // (the stream was synchronised above and nothing has been launched since)
    s->table_allocs.swap(fresh);
    s->device_bytes = s->device_bytes - s->table_bytes + fresh_bytes;
    s->table_bytes = fresh_bytes;
    s->dev = nd;
    s->uses_perlin = P.M.uses_perlin; s->max_image = P.M.max_image; s->bvh_node_count = P.bvh_node_count; s->bvh_depth = P.bvh_depth;
    s->host_kind = P.host_kind; s->media_fast_of = P.media_fast_of; s->mat = std::move(P.M); s->geom_ext = P.geom_ext;
    s->n_mats = a.n_mats; s->n_tex = a.n_tex;
    s->tree = std::move(P.tree);
    drop_geometry_edit(s); // the trees are new: nothing is displaced, and the refit plan was the old node array's
    return RTMI_OK;
}
int rebuild_for_camera(rtmi_scene *s, int cam_kind, const double *cam) {
    SceneArrays a = kept_arrays(s);
    a.cam_kind = cam_kind; a.cam = cam;
    const int rc = rebuild_scene(s, a, "rtmi_scene_set_camera");
    if (rc) return rc;
    s->args.cam.assign(cam, cam + 24); s->args.cam_kind = cam_kind;
    s->revision++;
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_scene_set_camera(rtmi_scene *s, int32_t cam_kind, const double *cam, int32_t *out_rebuilt) {
    int rc = check_camera_args(cam_kind, cam);
    if (rc) return rc;
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    double c24[24], t_lo, t_hi; // (a copy: the caller may hand back what rtmi_scene_camera gave it, or anything else that the call itself overwrites)
    std::memcpy(c24, cam, sizeof c24);
    HIP_TRY(hipSetDevice(s->ctx->device));
    if (!camera_fits(s, cam_kind, c24, &t_lo, &t_hi)) {
        rc = rebuild_for_camera(s, cam_kind, c24);
        if (!rc && out_rebuilt) *out_rebuilt = 1;
        return rc;
    }
    struct { int cam_kind, cam_fixed_origin; double cam[24]; } rec; // the descriptor's last three fields as they lie in it
    static_assert(sizeof rec == kCamBytes, "the camera range of the descriptor");
    rec.cam_kind = cam_kind; rec.cam_fixed_origin = camera_fixed_origin(cam_kind, c24);
    std::memcpy(rec.cam, c24, sizeof c24);
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    HIP_TRY(hipMemcpy((char *)(void *)s->d_dev + kCamOffset, &rec, kCamBytes, hipMemcpyHostToDevice));
    adopt_camera(s, cam_kind, c24);
    if (out_rebuilt) *out_rebuilt = 0;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_scene_set_camera_stream(rtmi_scene *s, int32_t cam_kind, const double *cam, void *stream) {
    int rc = check_camera_args(cam_kind, cam);
    if (rc) return rc;
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    CameraArgs a;
    std::memcpy(a.cam, cam, sizeof a.cam);
    a.cam_kind = cam_kind; a.cam_fixed_origin = camera_fixed_origin(cam_kind, a.cam);
    double t_lo, t_hi;
    if (!camera_fits(s, cam_kind, a.cam, &t_lo, &t_hi))
        return fail(RTMI_E_UNSUPPORTED, "the camera's shutter interval [%g, %g] lies outside the interval [%g, %g] the scene's MovingSphere bounds were built for: "
                                        "rtmi_scene_set_camera rebuilds them, the stream form does not", t_lo, t_hi, s->dev.cull_t_lo, s->dev.cull_t_hi);
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : s->ctx->stream;
    hipLaunchKernelGGL(set_camera_kernel, dim3(1), dim3(64), 0, st, (DevScene *)(void *)s->d_dev, a);
    HIP_TRY(hipGetLastError());
    adopt_camera(s, cam_kind, a.cam); // at once: the launch decisions of the renders queued behind the kernel (the stash's width) are taken at enqueue time
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_scene_camera(rtmi_scene *s, int32_t *cam_kind, double *cam, double *built_t_lo, double *built_t_hi) {
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    if (cam_kind) *cam_kind = s->dev.cam_kind;
    if (cam) std::memcpy(cam, s->dev.cam, 24 * sizeof(double));
    if (built_t_lo) *built_t_lo = s->dev.cull_t_lo;
    if (built_t_hi) *built_t_hi = s->dev.cull_t_hi;
    return RTMI_OK;
}

// ---- the materials and textures of a live scene (rtmi_scene_set_materials*) --------------------------------------------------------------------
namespace {
// One of the eleven tables that read the materials: its host copy in a PackedMaterials, its place in HBM, the bytes of one row
struct MatTable { const void *host; size_t bytes, row; const void *dev; };
constexpr int kMatTables = 11;
std::array<MatTable, kMatTables> material_tables(const PackedMaterials &M, const DevScene &d) {
    auto tab = [](const auto &v, size_t row_elems, const void *dev) { return MatTable{v.data(), v.size() * sizeof(v[0]), row_elems * sizeof(v[0]), dev}; };
    return {tab(M.mat_rec, 12, d.mat_rec), tab(M.mat_grad, 12, d.mat_grad), tab(M.mat_kind, 1, d.mat_kind), tab(M.mat_tex, 1, d.mat_tex),
            tab(M.mat_param, 1, d.mat_param), tab(M.tex_kind, 1, d.tex_kind), tab(M.tex_param, RTMI_TEX_STRIDE, d.tex_param), tab(M.tex_child, 2, d.tex_child),
            tab(M.prim_mat, 1, d.prim_mat), tab(M.prim_kind, 1, d.prim_kind), tab(M.prim_km, 2, d.prim_km)};
}

// The changed rows of a stream edit travel as kernel arguments: up to kPatchRows rows and kPatchWords 32-bit words of payload per launch (the argument space is
// 4 KiB).  Every table's rows are whole 32-bit words and 4-byte aligned in HBM.
constexpr int kPatchRows = 64, kPatchWords = 704;
struct PatchRow { unsigned *dst; unsigned short src, n; unsigned pad; }; // n words from word[src] to dst
struct PatchArgs { PatchRow row[kPatchRows]; unsigned word[kPatchWords]; int n_rows, pad; };
static_assert(sizeof(PatchArgs) <= 4096, "one launch's rows fit the kernel-argument space");
static_assert(RTMI_EDIT_STREAM_MAX_BYTES % 4 == 0 && 96 / 4 <= kPatchWords, "the largest row (MatRec, a texture's parameters: twelve doubles) fits one launch");

// One wave, in stream order: lane l stores row l, word by word.  Plain vector stores; the launch boundary orders them for the renders queued behind it on the
// stream (they read the tables through caches every kernel launch invalidates).  No LDS, no scratch.
__global__ void __launch_bounds__(64) set_materials_kernel(PatchArgs a) {
    const int l = (int)threadIdx.x;
    if (l >= a.n_rows) return;
    unsigned *dst = a.row[l].dst;
    const int src = a.row[l].src, n = a.row[l].n;
    for (int k = 0; k < n; ++k) dst[k] = a.word[src + k];
}

// the argument errors of both set forms, reported before the handle is examined
int check_material_arrays(int n_mats, const int32_t *mat_kind, const int32_t *mat_tex, const double *mat_param, int n_tex, const int32_t *tex_kind,
                          const double *tex_param, const int32_t *tex_child) {
    if (n_mats < 0 || n_tex < 0) return fail(RTMI_E_ARG, "negative count");
    if (n_mats > 0 && (!mat_kind || !mat_tex || !mat_param)) return fail(RTMI_E_ARG, "material arrays are NULL");
    if (n_tex > 0 && (!tex_kind || !tex_param || !tex_child)) return fail(RTMI_E_ARG, "texture arrays are NULL");
    return RTMI_OK;
}
// the checks creation applies to the materials, on the scene's arrays with the edited ones in their place
int check_material_edit(const SceneArrays &a) {
    int rc = check_material_tables(a);
    for (int i = 0; i < a.n_prims && !rc; ++i) {
        rc = check_prim_material(a, i);
        if (!rc && (a.prim_kind[i] & ~RTMI_PRIM_BOUNDARY) == RTMI_PRIM_MEDIUM) rc = check_medium_material(a, i);
    }
    return rc;
}
// The edit FITS the built scene: the tables keep their sizes and the scene keeps its kernels (dev.has_ext, and through it the entry grid and the small scan).
// why (optional): the reason it does not
bool materials_fit(const rtmi_scene *s, const SceneArrays &a, const PackedMaterials &M, std::string *why) {
    char buf[160] = "";
    const int has_ext = (s->geom_ext || M.has_ext) ? 1 : 0;
    if (a.n_mats != s->n_mats) snprintf(buf, sizeof buf, "the edit has %d materials, the scene %d", a.n_mats, s->n_mats);
    else if (a.n_tex != s->n_tex) snprintf(buf, sizeof buf, "the edit has %d textures, the scene %d", a.n_tex, s->n_tex);
    else if (has_ext != s->dev.has_ext)
        snprintf(buf, sizeof buf, "the edit %s a texture or material that only the EXT kernels hold (has_ext %d -> %d)", has_ext ? "brings in" : "removes the last use of", s->dev.has_ext, has_ext);
    else {
        const auto was = material_tables(s->mat, s->dev), now = material_tables(M, s->dev);
        for (int t = 0; t < kMatTables; ++t) if (was[(size_t)t].bytes != now[(size_t)t].bytes) snprintf(buf, sizeof buf, "table %d changes its size", t); // (cannot happen: the counts are equal)
    }
    if (why) *why = buf;
    return buf[0] == 0;
}
// the host's half of an edit: the mirror of the tables, the facts the render checks read, and the arguments a clone or a camera rebuild replays
void adopt_materials(rtmi_scene *s, const SceneArrays &a, PackedMaterials *M) {
    rtmi_scene::Args &A = s->args;
    if (M) { s->uses_perlin = M->uses_perlin; s->max_image = M->max_image; s->dev.defer_mat = M->defer_mat; s->mat = std::move(*M); } // (a rebuild has done this itself)
    if (a.prim_mat != A.prim_mat.data()) A.prim_mat.assign(a.prim_mat, a.prim_mat + a.n_prims);
    A.mat_kind.assign(a.mat_kind, a.mat_kind + a.n_mats); A.mat_tex.assign(a.mat_tex, a.mat_tex + a.n_mats); A.mat_param.assign(a.mat_param, a.mat_param + a.n_mats);
    A.tex_kind.assign(a.tex_kind, a.tex_kind + a.n_tex); A.tex_param.assign(a.tex_param, a.tex_param + (size_t)a.n_tex * RTMI_TEX_STRIDE);
    A.tex_child.assign(a.tex_child, a.tex_child + 2 * (size_t)a.n_tex);
    s->revision++;
}
// both forms up to the decision: the checks in the order they are reported, the scene's arrays with the edit in their place, the packed tables
int prepare_material_edit(rtmi_scene *s, int n_mats, const int32_t *mat_kind, const int32_t *mat_tex, const double *mat_param, int n_tex, const int32_t *tex_kind,
                          const double *tex_param, const int32_t *tex_child, const int32_t *prim_mat, SceneArrays &a, PackedMaterials &M) {
    int rc = check_material_arrays(n_mats, mat_kind, mat_tex, mat_param, n_tex, tex_kind, tex_param, tex_child);
    if (rc) return rc;
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    a = kept_arrays(s);
    a.n_mats = n_mats; a.mat_kind = mat_kind; a.mat_tex = mat_tex; a.mat_param = mat_param;
    a.n_tex = n_tex; a.tex_kind = tex_kind; a.tex_param = tex_param; a.tex_child = tex_child;
    if (prim_mat) a.prim_mat = prim_mat;
    rc = check_material_edit(a);
    if (rc) return rc;
    M = pack_materials(a, s->geom_ext);
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_scene_set_materials(rtmi_scene *s, int32_t n_mats, const int32_t *mat_kind, const int32_t *mat_tex, const double *mat_param,
                                         int32_t n_tex, const int32_t *tex_kind, const double *tex_param, const int32_t *tex_child,
                                         const int32_t *prim_mat, int32_t *out_rebuilt) {
    SceneArrays a;
    PackedMaterials M;
    int rc = prepare_material_edit(s, n_mats, mat_kind, mat_tex, mat_param, n_tex, tex_kind, tex_param, tex_child, prim_mat, a, M);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->ctx->device));
    if (!materials_fit(s, a, M, nullptr)) {
        rc = rebuild_scene(s, a, "rtmi_scene_set_materials");
        if (rc) return rc;
        adopt_materials(s, a, nullptr);
        if (out_rebuilt) *out_rebuilt = 1;
        return RTMI_OK;
    }
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    const auto was = material_tables(s->mat, s->dev), now = material_tables(M, s->dev);
    for (int t = 0; t < kMatTables; ++t) { // each table where it lies; a table the edit leaves as it is does not travel
        const MatTable &o = was[(size_t)t], &n = now[(size_t)t];
        if (n.bytes == 0 || std::memcmp(o.host, n.host, n.bytes) == 0) continue;
        HIP_TRY(hipMemcpy(const_cast<void *>(n.dev), n.host, n.bytes, hipMemcpyHostToDevice));
    }
    adopt_materials(s, a, &M);
    if (out_rebuilt) *out_rebuilt = 0;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_scene_set_materials_stream(rtmi_scene *s, int32_t n_mats, const int32_t *mat_kind, const int32_t *mat_tex, const double *mat_param,
                                                int32_t n_tex, const int32_t *tex_kind, const double *tex_param, const int32_t *tex_child,
                                                const int32_t *prim_mat, void *stream) {
    SceneArrays a;
    PackedMaterials M;
    int rc = prepare_material_edit(s, n_mats, mat_kind, mat_tex, mat_param, n_tex, tex_kind, tex_param, tex_child, prim_mat, a, M);
    if (rc) return rc;
    std::string why;
    if (!materials_fit(s, a, M, &why))
        return fail(RTMI_E_UNSUPPORTED, "%s: rtmi_scene_set_materials rebuilds the scene for such an edit, the stream form does not", why.c_str());
    // the rows that differ from the mirror, batched into launches
    const auto was = material_tables(s->mat, s->dev), now = material_tables(M, s->dev);
    std::vector<PatchArgs> batches;
    size_t payload = 0;
    int words_used = 0;
    for (int t = 0; t < kMatTables; ++t) {
        const MatTable &o = was[(size_t)t], &n = now[(size_t)t];
        const char *ob = (const char *)o.host, *nb = (const char *)n.host;
        for (size_t off = 0; off + n.row <= n.bytes; off += n.row) {
            if (std::memcmp(ob + off, nb + off, n.row) == 0) continue;
            payload += n.row;
            if (payload > RTMI_EDIT_STREAM_MAX_BYTES)
                return fail(RTMI_E_UNSUPPORTED, "the edit changes more than RTMI_EDIT_STREAM_MAX_BYTES = %d bytes of table rows: rtmi_scene_set_materials copies whole tables, "
                                                "the stream form is for the few records an interactive edit touches", RTMI_EDIT_STREAM_MAX_BYTES);
            const int nw = (int)(n.row / 4);
            if (batches.empty() || batches.back().n_rows == kPatchRows || words_used + nw > kPatchWords) {
                batches.emplace_back();
                std::memset(&batches.back(), 0, sizeof(PatchArgs));
                words_used = 0;
            }
            PatchArgs &b = batches.back();
            PatchRow &r = b.row[b.n_rows++];
            r.dst = reinterpret_cast<unsigned *>(const_cast<char *>((const char *)n.dev + off));
            r.src = (unsigned short)words_used; r.n = (unsigned short)nw;
            std::memcpy(&b.word[words_used], nb + off, n.row);
            words_used += nw;
        }
    }
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : s->ctx->stream;
    for (const PatchArgs &b : batches) {
        hipLaunchKernelGGL(set_materials_kernel, dim3(1), dim3(64), 0, st, b);
        HIP_TRY(hipGetLastError());
    }
    adopt_materials(s, a, &M); // at once, like the camera's mirror: the render checks (Perlin table, images) of the calls queued behind the kernel read it
    return RTMI_OK;
}

// test hook, host code only (no device): the eleven material tables of the given arrays as rtmi_scene_set_materials* packs them (through_creation = 0: only the
// primitive kinds and materials and the material and texture tables are read, the other arrays may be NULL) or as rtmi_scene_create_ex does (1: through its
// checks and pack_scene).  out_hash = FNV-1a of the tables, out_facts = {the materials' share of has_ext, uses_perlin, max_image}
RTMI_EXPORT int rtmi_test_pack_materials(int32_t n_prims, const int32_t *prim_kind, const double *prim_geom, const int32_t *prim_mat,
                                         int32_t n_mats, const int32_t *mat_kind, const int32_t *mat_tex, const double *mat_param,
                                         int32_t n_tex, const int32_t *tex_kind, const double *tex_param, const int32_t *tex_child,
                                         int32_t cam_kind, const double *cam, const int32_t *prim_flip, const int32_t *prim_xform,
                                         int32_t n_xforms, const int32_t *xform_kind, const double *xform_param, int32_t through_creation,
                                         uint64_t *out_hash, int32_t *out_facts) {
    if (!out_hash || !out_facts) return fail(RTMI_E_ARG, "bad arguments");
    const SceneArrays a{n_prims, prim_kind, prim_geom, prim_mat, n_mats, mat_kind, mat_tex, mat_param, n_tex, tex_kind, tex_param, tex_child,
                        cam_kind, cam, prim_flip, prim_xform, n_xforms, xform_kind, xform_param};
    PackedMaterials M;
    if (through_creation) {
        rtmi_scene *none = nullptr;
        const int rc = check_scene_args(a, &none);
        if (rc) return rc;
        M = pack_scene(a, read_build_knobs()).M;
    } else {
        int rc = check_material_arrays(n_mats, mat_kind, mat_tex, mat_param, n_tex, tex_kind, tex_param, tex_child);
        if (!rc && (n_prims < 0 || (n_prims > 0 && (!prim_kind || !prim_mat)))) rc = fail(RTMI_E_ARG, "primitive arrays are NULL");
        if (!rc) rc = check_material_edit(a);
        if (rc) return rc;
        M = pack_materials(a, geometry_is_ext(a)); // (no built scene to ask: the hook reads the arrays)
    }
    uint64_t h = 1469598103934665603ull;
    DevScene none{};
    for (const MatTable &t : material_tables(M, none)) {
        const unsigned char *q = (const unsigned char *)t.host;
        for (size_t k = 0; k < t.bytes; ++k) { h ^= q[k]; h *= 1099511628211ull; }
        h ^= (uint64_t)t.bytes; h *= 1099511628211ull;
    }
    *out_hash = h;
    out_facts[0] = M.has_ext ? 1 : 0; out_facts[1] = M.uses_perlin ? 1 : 0; out_facts[2] = M.max_image;
    return RTMI_OK;
}

// ---- the geometry of a live scene (rtmi_scene_set_geometry) ------------------------------------------------------------------------------------
// The trees keep their topology; every box plane is recomputed bottom-up from the leaves.  BvhBuilder::put_box and half_outward are monotone, so a
// union of rounded boxes is the rounded union: for the same topology the refit writes the planes the builder would.
namespace {
// Box planes travel as BITS (a float's, or a half's) and are compared by a key that orders them like their values, -0 below +0; nothing here needs libm.
__host__ __device__ inline int refit_key32(unsigned u) { const int v = (int)u; return v ^ ((v >> 31) & 0x7fffffff); }
__host__ __device__ inline int refit_key16(unsigned h) { const int v = (int)(short)(unsigned short)h; return v ^ ((v >> 31) & 0x7fff); }
// half_outward (scene_build.h) on a float's bits, subnormal halves included in integer arithmetic: the same half for every input (rtmi_test_refit_half)
__host__ __device__ inline unsigned refit_half_outward(unsigned u, bool up) {
    const unsigned sign = u >> 31, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return 0x7e00u | (sign << 15); // NaN
    const bool away = up != (sign != 0);
    unsigned m;
    bool inexact;
    if (a >= 0x47800000u) { m = a == 0x7f800000u ? 0x7c00u : 0x7bffu; inexact = a != 0x7f800000u; }
    else if (a >= 0x38800000u) { m = (((a >> 23) - 112u) << 10) | ((a & 0x7fffffu) >> 13); inexact = (a & 0x1fffu) != 0; }
    else { // half subnormals, units of 2^-24: |x| = mant 2^(e - 150), so m = mant >> (126 - e)
        const unsigned e = a >> 23, mant = (a & 0x7fffffu) | 0x800000u, sh = 126u - e;
        if (e == 0 || sh >= 25u) { m = 0; inexact = a != 0; }
        else { m = mant >> sh; inexact = (mant & ((1u << sh) - 1u)) != 0; }
    }
    if (inexact && away) m += 1;
    return m | (sign << 15);
}
// record layouts (BvhBuilder::put_box; Node16): plane (side, axis k, hi) of a record's words, and the words of its two child codes
template <bool H> __host__ __device__ inline unsigned refit_get(const unsigned *w, int side, int k, int hi) {
    if (H) { const int h = side * 6 + k * 2 + hi; return (w[h >> 1] >> ((h & 1) * 16)) & 0xffffu; }
    return k < 2 ? w[side * 4 + hi * 2 + k] : w[8 + side * 2 + hi];
}
template <bool H> __host__ __device__ inline void refit_put(unsigned *w, int side, int k, int hi, unsigned v) {
    if (H) { const int h = side * 6 + k * 2 + hi; w[h >> 1] = (h & 1) ? ((w[h >> 1] & 0xffffu) | (v << 16)) : ((w[h >> 1] & 0xffff0000u) | v); }
    else w[k < 2 ? side * 4 + hi * 2 + k : 8 + side * 2 + hi] = v;
}
template <bool H> __host__ __device__ inline void refit_load(const unsigned *p, unsigned *w) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
#pragma unroll
    for (int k = 0; k < (H ? 2 : 4); ++k) { const uint4 v = q[k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
#else
    for (int k = 0; k < (H ? 8 : 16); ++k) w[k] = p[k];
#endif
}
// One node: both boxes from its children -- RTMI_BVH_EMPTY, or the right side of a lone primitive's node: the empty box; a leaf: leaf_box[primitive] (the moving and Box bits masked off, as the traversal
// does), through half_outward for half records; an inner child: the union of that record's two boxes, refit before (its height is lower).  The child codes are
// read, never written.  nodes: the whole array as 32-bit words.
template <bool H> __host__ __device__ inline void refit_node(unsigned *nodes, const float *leaf_box, int n) {
    constexpr int REC = H ? 8 : 16, CODE = H ? 6 : 12; // words per record, word of the left child code
    unsigned own[16], out[12];
    refit_load<H>(nodes + (size_t)n * REC, own);
#pragma unroll
    for (int k = 0; k < 12; ++k) out[k] = own[k];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const int code = (int)own[CODE + side];
        unsigned lo[3], hi[3];
        if (code >= 0) {
            unsigned ch[16];
            refit_load<H>(nodes + (size_t)code / 4, ch);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const unsigned l0 = refit_get<H>(ch, 0, k, 0), l1 = refit_get<H>(ch, 1, k, 0), h0 = refit_get<H>(ch, 0, k, 1), h1 = refit_get<H>(ch, 1, k, 1);
                if (H) { lo[k] = refit_key16(l1) < refit_key16(l0) ? l1 : l0; hi[k] = refit_key16(h1) > refit_key16(h0) ? h1 : h0; }
                else { lo[k] = refit_key32(l1) < refit_key32(l0) ? l1 : l0; hi[k] = refit_key32(h1) > refit_key32(h0) ? h1 : h0; }
            }
        } else {
            unsigned fl[3] = {0x7f800000u, 0x7f800000u, 0x7f800000u}, fh[3] = {0xff800000u, 0xff800000u, 0xff800000u}; // +inf, -inf
            // (a tree over ONE primitive, BvhBuilder::lone, names its leaf on both sides and gives the right side the empty box: no build puts a leaf twice otherwise)
            if (code != RTMI_BVH_EMPTY && !(side == 1 && code == (int)own[CODE])) {
                const unsigned *b = reinterpret_cast<const unsigned *>(leaf_box) + (size_t)(~code & 0x1fffffff) * 6;
#pragma unroll
                for (int k = 0; k < 3; ++k) { fl[k] = b[k]; fh[k] = b[3 + k]; }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) { lo[k] = H ? refit_half_outward(fl[k], false) : fl[k]; hi[k] = H ? refit_half_outward(fh[k], true) : fh[k]; }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) { refit_put<H>(out, side, k, 0, lo[k]); refit_put<H>(out, side, k, 1, hi[k]); }
    }
    unsigned *dst = nodes + (size_t)n * REC;
#if defined(__HIP_DEVICE_COMPILE__)
    uint4 *q = reinterpret_cast<uint4 *>(dst);
    q[0] = make_uint4(out[0], out[1], out[2], out[3]);
    if (H) *reinterpret_cast<uint2 *>(dst + 4) = make_uint2(out[4], out[5]);
    else { q[1] = make_uint4(out[4], out[5], out[6], out[7]); q[2] = make_uint4(out[8], out[9], out[10], out[11]); }
#else
    for (int k = 0; k < (H ? 6 : 12); ++k) dst[k] = out[k];
#endif
}

// One launch per height, lowest first, in stream order: thread i refits node order[i].  The nodes of one height read only records of lower heights (written by
// earlier launches) and their own child codes (never written): the launch boundary is the only ordering.  Plain vector stores, no LDS, no atomics.
struct RefitArgs { unsigned *nodes; const float *leaf_box; const int *order; int count, node16; };
__global__ void __launch_bounds__(256) refit_kernel(RefitArgs a) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= a.count) return;
    const int n = a.order[i];
    if (a.node16) refit_node<true>(a.nodes, a.leaf_box, n);
    else refit_node<false>(a.nodes, a.leaf_box, n);
}

// The refit plan of a node array: every node's height (0: no inner child), the node indices sorted by height.  It also proves what the kernel relies on: every
// inner child is a record of the array BEHIND its parent (BvhBuilder::build allocates a node before it recurses; the rectangle trees are rebased as blocks), and
// every leaf names a world primitive.  false: the array is not of that form (the edit rebuilds).
bool make_refit_plan(const unsigned *w, int n_nodes, bool node16, int n_world, std::vector<int> &order, std::vector<int> &level_off) {
    const int rec = node16 ? 8 : 16, code_at = node16 ? 6 : 12;
    std::vector<int> height((size_t)n_nodes, 0);
    int top = -1;
    for (int n = n_nodes - 1; n >= 0; --n) {
        int h = 0;
        for (int side = 0; side < 2; ++side) {
            const int c = (int)w[(size_t)n * rec + code_at + side];
            if (c == RTMI_BVH_EMPTY) continue;
            if (c < 0) { if ((~c & 0x1fffffff) >= n_world) return false; continue; }
            const int ci = c / (rec * 4);
            if (c % (rec * 4) != 0 || ci <= n || ci >= n_nodes) return false;
            h = std::max(h, height[(size_t)ci] + 1);
        }
        height[(size_t)n] = h;
        top = std::max(top, h);
    }
    level_off.assign((size_t)top + 2, 0);
    for (int n = 0; n < n_nodes; ++n) level_off[(size_t)height[(size_t)n] + 1]++;
    for (size_t h = 1; h < level_off.size(); ++h) level_off[h] += level_off[h - 1];
    order.resize((size_t)n_nodes);
    std::vector<int> at(level_off.begin(), level_off.end() - 1);
    for (int n = 0; n < n_nodes; ++n) order[(size_t)at[(size_t)height[(size_t)n]]++] = n;
    return true;
}
// the host's refit, level by level as the device runs it: the reference the kernel is compared with (rtmi_test_refit)
void refit_host(unsigned *w, bool node16, const float *leaf_box, const std::vector<int> &order) {
    for (int n : order) { if (node16) refit_node<true>(w, leaf_box, n); else refit_node<false>(w, leaf_box, n); }
}

// What an edit of the geometry does to a built scene (see rtmi.h).  The built state: the TreeBuild record, the descriptor's rounded bounds, the kinds, the
// geometry and bounded flags in HBM, who is displaced already.  The edit: its arrays and their world boxes (packed with the BUILT shutter interval).
struct GeoVerdict {
    bool fits = false;
    std::string why;
    std::vector<char> displaced;
    int n_displaced = 0, n_big = 0, big_idx[16] = {0};
    std::vector<float> leaf_box;
};
GeoVerdict judge_geometry(const TreeBuild &T, const DevScene &d, const std::vector<int> &kind, int n_world, const double *geom_was, const std::vector<char> &bounded_was,
                          const double *geom_now, const GeomExtras &X, const std::vector<char> &displaced_was) {
    GeoVerdict V;
    char buf[200] = "";
    const int n_prims = (int)kind.size();
    const double ob = (double)d.bvh_obound, cb = (double)d.bvh_cbound;
    V.displaced = displaced_was;
    V.displaced.resize((size_t)std::max(n_world, 1), 0);
    V.leaf_box.assign((size_t)std::max(n_world, 1) * 6, 0.0f);
    if (T.box_leaves) snprintf(buf, sizeof buf, "the tree holds Box leaves (RTMI_BOX_LEAF)");
    else if (d.n_mloc) snprintf(buf, sizeof buf, "the scene has media neighbourhood trees (RTMI_MLOC)");
    for (int i = 0; i < n_prims && !buf[0]; ++i) {
        if (kind[(size_t)i] == RTMI_PRIM_MEDIUM) {
            if (std::memcmp(geom_was + (size_t)i * RTMI_PRIM_STRIDE, geom_now + (size_t)i * RTMI_PRIM_STRIDE, RTMI_PRIM_STRIDE * sizeof(double)) != 0)
                snprintf(buf, sizeof buf, "medium %d changes (its density and boundary range are structure)", i);
            continue;
        }
        if (X.bounded[(size_t)i] != bounded_was[(size_t)i]) { snprintf(buf, sizeof buf, "primitive %d %s be bounded", i, X.bounded[(size_t)i] ? "can now" : "can no longer"); break; }
        if (i >= n_world) continue; // boundary primitives are in no tree
        const unsigned char cls = T.cls[(size_t)i];
        const BvhBox b = tree_item_box(X.bounded[(size_t)i] != 0, X.wbox[(size_t)i]);
        float *lbx = &V.leaf_box[(size_t)i * 6];
        for (int k = 0; k < 3; ++k) { lbx[k] = INFINITY; lbx[3 + k] = -INFINITY; }
        if (X.bounded[(size_t)i])
            for (int k = 0; k < 3 && !buf[0]; ++k)
                if (!(std::fabs(b.lo[k]) <= ob && std::fabs(b.hi[k]) <= ob)) snprintf(buf, sizeof buf, "primitive %d leaves the bound %g the trees were built for", i, ob);
        if (buf[0] || !(cls & TB_ITEM)) continue;
        for (int k = 0; k < 3 && !buf[0]; ++k)
            if (!(std::fabs(b.lo[k]) <= cb && std::fabs(b.hi[k]) <= cb)) snprintf(buf, sizeof buf, "tree primitive %d leaves the bound %g of the boxes in the tree", i, cb);
        if (buf[0]) break;
        if (T.grid && !V.displaced[(size_t)i]) {
            bool out = false;
            if (cls & TB_LAYER) {
                int r[4];
                grid_cell_range(b, T.lb, T.G, T.csx, T.csz, T.eps, r);
                const int *c = &T.cell[(size_t)i * 4];
                out = r[0] < c[0] || r[1] > c[1] || r[2] < c[2] || r[3] > c[3];
                for (int k = 0; k < 3; ++k) out = out || !(b.lo[k] >= T.lb.lo[k] && b.hi[k] <= T.lb.hi[k]);
            } else if (cls & TB_TALL)
                for (int k = 0; k < 3; ++k) out = out || !(b.lo[k] >= T.tb.lo[k] && b.hi[k] <= T.tb.hi[k]);
            if (out) V.displaced[(size_t)i] = 1;
        }
        if (!V.displaced[(size_t)i]) // BvhBuilder::put_box
            for (int k = 0; k < 3; ++k) { lbx[k] = f_down(b.lo[k] - T.delta); lbx[3 + k] = f_up(b.hi[k] + T.delta); }
    }
    if (!buf[0]) { // the big list: the build's and the displaced, ascending
        int total = 0;
        for (int i = 0; i < n_world; ++i) {
            const bool big = (T.cls[(size_t)i] & TB_BIG) || V.displaced[(size_t)i];
            if (V.displaced[(size_t)i]) V.n_displaced++;
            if (!big) continue;
            if (total < 16) V.big_idx[total] = i;
            total++;
        }
        V.n_big = std::min(total, 16);
        if (total > 16) snprintf(buf, sizeof buf, "%d displaced primitives: the big list would hold %d entries, it has 16", V.n_displaced, total);
    }
    V.why = buf;
    V.fits = buf[0] == 0;
    return V;
}

// the geometry tables that lie in HBM where an edit rewrites them: host copy in a PackedScene, place in the descriptor
struct GeoTable { const void *host; size_t bytes; const void *dev; };
constexpr int kGeoTables = 8;
std::array<GeoTable, kGeoTables> geometry_tables(const PackedScene &P, const DevScene &d) {
    auto tab = [](const auto &v, const void *dev) { return GeoTable{v.data(), v.size() * sizeof(v[0]), dev}; };
    return {tab(P.stat_geom, d.stat_geom), tab(P.stat4_d, d.stat4_d), tab(P.stat4_f, d.stat4_f), tab(P.exact12, d.exact12), tab(P.cull20, d.cull20),
            tab(P.leaf_rec, d.leaf_rec), tab(P.ext_xf, d.ext_xf), tab(P.mov_geom, d.mov_geom)};
}
uint64_t hash_geometry(const PackedScene &P, const GeomExtras &X) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void *p, size_t bytes) { const unsigned char *q = (const unsigned char *)p; for (size_t k = 0; k < bytes; ++k) { h ^= q[k]; h *= 1099511628211ull; } h ^= (uint64_t)bytes; h *= 1099511628211ull; };
    DevScene none{};
    for (const GeoTable &t : geometry_tables(P, none)) mix(t.host, t.bytes);
    for (const auto &kv : P.media_fast_of) { mix(&kv.first, sizeof(int)); mix(kv.second.data(), 5 * sizeof(double)); }
    mix(X.bounded.data(), X.bounded.size());
    for (size_t i = 0; i < X.wbox.size(); ++i) if (X.bounded[i]) mix(&X.wbox[i], sizeof(BvhBox));
    return h;
}
void pack_geometry_only(const SceneArrays &a, double t_lo, double t_hi, PackedScene &P, GeomExtras &X) {
    std::memset(&P.d, 0, sizeof P.d);
    pack_geometry(a, read_build_knobs().box_leaf, t_lo, t_hi, P, X);
}
// the first edit after a build: the mirror of the tables, the refit plan and the two device tables that go with it
int prepare_geometry_edit(rtmi_scene *s) {
    rtmi_scene::GeoEdit &g = s->geo;
    if (g.ready) return RTMI_OK;
    const DevScene &d = s->dev;
    pack_geometry_only(kept_arrays(s), d.cull_t_lo, d.cull_t_hi, g.tab, g.X);
    g.displaced.assign((size_t)std::max(d.n_all, 1), 0);
    g.leaf_box.assign((size_t)std::max(d.n_all, 1) * 6, 0.0f);
    std::vector<int> order;
    const int n_nodes = d.bvh_root == RTMI_BVH_EMPTY && !d.grid_n ? 0 : s->bvh_node_count;
    if (n_nodes > 0) {
        std::vector<unsigned> w((size_t)n_nodes * (d.bvh_node16 ? 8 : 16));
        HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        HIP_TRY(hipMemcpy(w.data(), d.bvh_nodes, w.size() * 4, hipMemcpyDeviceToHost));
        if (!make_refit_plan(w.data(), n_nodes, d.bvh_node16 != 0, d.n_all, order, g.level_off)) return fail(RTMI_E_STATE, "the scene's node array is not in parent-before-child order");
    }
    const size_t ob = std::max(order.size(), (size_t)1) * sizeof(int), lb = g.leaf_box.size() * sizeof(float);
    if (hipMalloc((void **)&g.d_order, ob) != hipSuccess || hipMalloc((void **)&g.d_leaf_box, lb) != hipSuccess) {
        if (g.d_order) (void)hipFree(g.d_order);
        g = rtmi_scene::GeoEdit();
        return fail(RTMI_E_NOMEM, "hipMalloc(%zu) failed", ob + lb);
    }
    g.bytes = ob + lb;
    s->device_bytes += g.bytes;
    if (!order.empty()) HIP_TRY(hipMemcpy(g.d_order, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice));
    if (s->ctx->flags & RTMI_FLAG_TIMING) { HIP_TRY(hipEventCreate(&g.ev0)); HIP_TRY(hipEventCreate(&g.ev1)); }
    g.ready = true;
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_scene_set_geometry(rtmi_scene *s, int32_t n_prims, const double *prim_geom, int32_t n_xforms, const double *xform_param, int32_t mode, int32_t *out_info) {
    if (n_prims < 0 || n_xforms < 0) return fail(RTMI_E_ARG, "negative count");
    if (n_prims > 0 && !prim_geom) return fail(RTMI_E_ARG, "primitive arrays are NULL");
    if (mode != 0 && mode != 1) return fail(RTMI_E_ARG, "mode must be 0 (in place if the edit fits) or 1 (rebuild)");
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    if (n_prims != s->n_prims || n_xforms != (int)s->args.xform_kind.size())
        return fail(RTMI_E_ARG, "the edit has %d primitives and %d instance records, the scene %d and %d: a changed count or kind is a new scene", n_prims, n_xforms, s->n_prims,
                    (int)s->args.xform_kind.size());
    SceneArrays a = kept_arrays(s);
    a.prim_geom = prim_geom;
    if (xform_param && n_xforms > 0) a.xform_param = xform_param;
    rtmi_scene *none = nullptr;
    int rc = check_scene_args(a, &none); // creation's checks of the same arrays, with its codes
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->ctx->device));
    int info[4] = {0, 0, 0, 0};
    PackedScene P;
    GeomExtras X;
    GeoVerdict V;
    if (mode == 0) {
        rc = prepare_geometry_edit(s);
        if (rc) return rc;
        pack_geometry_only(a, s->dev.cull_t_lo, s->dev.cull_t_hi, P, X);
        V = judge_geometry(s->tree, s->dev, s->host_kind, s->dev.n_all, s->args.prim_geom.data(), s->geo.X.bounded, prim_geom, X, s->geo.displaced);
    }
    rtmi_scene::Args &A = s->args;
    auto adopt = [&]() { // (after the last use of `a`, which may point into the arrays replaced here)
        if (prim_geom != A.prim_geom.data()) A.prim_geom.assign(prim_geom, prim_geom + (size_t)n_prims * RTMI_PRIM_STRIDE);
        if (xform_param && n_xforms > 0 && xform_param != A.xform_param.data()) A.xform_param.assign(xform_param, xform_param + 3 * (size_t)n_xforms);
        s->revision++;
    };
    if (!V.fits) {
        rc = rebuild_scene(s, a, "rtmi_scene_set_geometry");
        if (rc) return rc;
        adopt();
        info[0] = 1;
        if (out_info) std::memcpy(out_info, info, sizeof info);
        return RTMI_OK;
    }
    rtmi_scene::GeoEdit &g = s->geo;
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    const auto was = geometry_tables(g.tab, s->dev), now = geometry_tables(P, s->dev);
    for (int t = 0; t < kGeoTables; ++t) { // each table where it lies; a table the edit leaves as it is does not travel
        const GeoTable &o = was[(size_t)t], &n = now[(size_t)t];
        if (o.bytes != n.bytes) return fail(RTMI_E_STATE, "geometry table %d changes its size", t); // (cannot happen: kinds, flips and chains are the scene's)
        if (n.bytes == 0 || std::memcmp(o.host, n.host, n.bytes) == 0) continue;
        HIP_TRY(hipMemcpy(const_cast<void *>(n.dev), n.host, n.bytes, hipMemcpyHostToDevice));
    }
    DevScene nd = s->dev;
    nd.n_big = V.n_big;
    for (int k = 0; k < 16; ++k) nd.big_idx[k] = k < V.n_big ? V.big_idx[k] : 0;
    fill_media_fast(nd, P.media_fast_of);
    if (std::memcmp(&nd, &s->dev, sizeof nd) != 0) HIP_TRY(hipMemcpy((void *)s->d_dev, &nd, sizeof(DevScene), hipMemcpyHostToDevice));
    const int n_nodes = g.level_off.empty() ? 0 : g.level_off.back();
    if (n_nodes > 0) {
        HIP_TRY(hipMemcpy(g.d_leaf_box, V.leaf_box.data(), V.leaf_box.size() * sizeof(float), hipMemcpyHostToDevice));
        if (g.ev0) HIP_TRY(hipEventRecord(g.ev0, s->ctx->stream));
        for (size_t h = 0; h + 1 < g.level_off.size(); ++h) {
            const int count = g.level_off[h + 1] - g.level_off[h];
            if (count <= 0) continue;
            const RefitArgs ra{reinterpret_cast<unsigned *>(const_cast<void *>((const void *)nd.bvh_nodes)), g.d_leaf_box, g.d_order + g.level_off[h], count, nd.bvh_node16};
            hipLaunchKernelGGL(refit_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s->ctx->stream, ra);
            HIP_TRY(hipGetLastError());
            info[3]++;
        }
        info[2] = n_nodes;
        if (g.ev1) { HIP_TRY(hipEventRecord(g.ev1, s->ctx->stream)); g.timed = true; }
    }
    s->dev = nd;
    s->media_fast_of = P.media_fast_of;
    g.leaf_box.swap(V.leaf_box);
    g.displaced.swap(V.displaced);
    g.tab = std::move(P);
    g.X = std::move(X);
    adopt();
    info[1] = V.n_displaced;
    if (out_info) std::memcpy(out_info, info, sizeof info);
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_scene_last_refit_ms(rtmi_scene *s, double *out_ms) {
    if (!out_ms) return fail(RTMI_E_ARG, "out_ms is NULL");
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    if (!s->geo.timed) return fail(RTMI_E_STATE, "no timed refit: the context needs RTMI_FLAG_TIMING and the scene an in-place rtmi_scene_set_geometry since its last build");
    HIP_TRY(hipSetDevice(s->ctx->device));
    HIP_TRY(hipEventSynchronize(s->geo.ev1));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, s->geo.ev0, s->geo.ev1));
    *out_ms = (double)ms;
    return RTMI_OK;
}

// test hook, host code only (no device): the geometry tables of the given arrays as creation packs them (through_creation = 1: its checks, then pack_scene) or
// as rtmi_scene_set_geometry does (0: pack_geometry alone, with the camera's shutter interval).  out_hash = FNV-1a of stat_geom, stat4_d, stat4_f, exact12,
// cull20, leaf_rec, ext_xf, mov_geom, media_fast_of and every primitive's bounded flag and world box.
RTMI_EXPORT int rtmi_test_pack_geometry(int32_t n_prims, const int32_t *prim_kind, const double *prim_geom, const int32_t *prim_mat,
                                        int32_t n_mats, const int32_t *mat_kind, const int32_t *mat_tex, const double *mat_param,
                                        int32_t n_tex, const int32_t *tex_kind, const double *tex_param, const int32_t *tex_child,
                                        int32_t cam_kind, const double *cam, const int32_t *prim_flip, const int32_t *prim_xform,
                                        int32_t n_xforms, const int32_t *xform_kind, const double *xform_param, int32_t through_creation, uint64_t *out_hash) {
    if (!out_hash) return fail(RTMI_E_ARG, "bad arguments");
    const SceneArrays a{n_prims, prim_kind, prim_geom, prim_mat, n_mats, mat_kind, mat_tex, mat_param, n_tex, tex_kind, tex_param, tex_child,
                        cam_kind, cam, prim_flip, prim_xform, n_xforms, xform_kind, xform_param};
    rtmi_scene *none = nullptr;
    const int rc = check_scene_args(a, &none);
    if (rc) return rc;
    double t_lo, t_hi;
    camera_shutter(cam_kind, cam, t_lo, t_hi);
    if (through_creation) {
        // (pack_scene keeps no world boxes: they are recomputed here by the function it calls)
        const PackedScene P = pack_scene(a, read_build_knobs());
        PackedScene Q;
        GeomExtras X;
        pack_geometry_only(a, t_lo, t_hi, Q, X);
        *out_hash = hash_geometry(P, X);
    } else {
        PackedScene P;
        GeomExtras X;
        pack_geometry_only(a, t_lo, t_hi, P, X);
        *out_hash = hash_geometry(P, X);
    }
    return RTMI_OK;
}

// test hook, host code only (no device): the trees of geometry 0 as creation builds them, then n_steps - 1 edits as rtmi_scene_set_geometry applies them, the
// refit done by the host's reference (refit_host).  geoms = [n_steps][n_prims][RTMI_PRIM_STRIDE], xforms = [n_steps][n_xforms][3] (NULL with n_xforms = 0); the
// scene's surfaces are one grey Lambertian, its media Isotropic: every primitive goes through the kernels its geometry asks for.  Outputs, all of the state after the last step: the node array,
// out_info = {node16, bvh_root, grid_tall, grid cells per side, n_big, displaced, rebuilt by the last step, node records, refit launches, steps that rebuilt},
// out_big[16], the 4 G G root codes of the grid (up to cells_capacity), leaf_box [n_world][6] of the last in-place step (optional).
RTMI_EXPORT int rtmi_test_refit(int32_t n_prims, const int32_t *prim_kind, const int32_t *prim_flip, const int32_t *prim_xform, int32_t n_xforms, const int32_t *xform_kind,
                                int32_t cam_kind, const double *cam, int32_t n_steps, const double *geoms, const double *xforms,
                                void *out_nodes, int64_t capacity, int64_t *out_bytes, int32_t *out_info, int32_t *out_big,
                                int32_t *out_cells, int64_t cells_capacity, void *out_leaf_box) {
    if (n_prims <= 0 || !prim_kind || !cam || n_steps < 1 || !geoms || !out_bytes || !out_info || n_xforms < 0 || (n_xforms > 0 && (!xforms || !xform_kind || !prim_xform)))
        return fail(RTMI_E_ARG, "bad arguments");
    const BuildKnobs K = read_build_knobs();
    std::vector<int32_t> mat((size_t)n_prims, 0); // a grey Lambertian; the media scatter by material 1
    for (int i = 0; i < n_prims; ++i) mat[(size_t)i] = (prim_kind[i] & ~RTMI_PRIM_BOUNDARY) == RTMI_PRIM_MEDIUM ? 1 : 0;
    const int32_t mk[2] = {RTMI_MAT_LAMBERTIAN, RTMI_MAT_ISOTROPIC}, mt[2] = {0, 0}, tk = RTMI_TEX_CONSTANT, tc[2] = {-1, -1};
    const double mp[2] = {0.0, 0.0}, tp[RTMI_TEX_STRIDE] = {0.5, 0.5, 0.5};
    auto arrays = [&](int step) {
        return SceneArrays{n_prims, prim_kind, geoms + (size_t)step * n_prims * RTMI_PRIM_STRIDE, mat.data(), 2, mk, mt, mp, 1, &tk, tp, tc, cam_kind, cam, prim_flip, prim_xform,
                           n_xforms, xform_kind, n_xforms ? xforms + (size_t)step * n_xforms * 3 : nullptr};
    };
    PackedScene S; // the scene: its trees, its tables
    GeomExtras SX;
    std::vector<char> displaced;
    std::vector<int> order, level_off;
    std::vector<float> leaf_box;
    int n_nodes = 0, displaced_n = 0, rebuilt_last = 0, rebuilds = 0, launches = 0;
    const double *geom_was = nullptr;
    auto build = [&](int step) -> int {
        const SceneArrays a = arrays(step);
        rtmi_scene *none = nullptr;
        const int rc = check_scene_args(a, &none);
        if (rc) return rc;
        S = PackedScene();
        std::memset(&S.d, 0, sizeof S.d);
        double t_lo, t_hi;
        camera_shutter(cam_kind, cam, t_lo, t_hi);
        pack_geometry(a, K.box_leaf, t_lo, t_hi, S, SX);
        build_trees(a, K, S.geom_ext, SX, S);
        S.bvh_node_count = (int)(S.bvh_nodes.size() / (S.d.bvh_node16 ? 8 : 16));
        n_nodes = S.d.bvh_root == RTMI_BVH_EMPTY && !S.d.grid_n ? 0 : S.bvh_node_count;
        displaced.assign((size_t)std::max(S.d.n_all, 1), 0);
        leaf_box.assign((size_t)std::max(S.d.n_all, 1) * 6, 0.0f);
        displaced_n = 0; launches = 0;
        order.clear(); level_off.clear();
        geom_was = a.prim_geom;
        if (n_nodes > 0 && !make_refit_plan(reinterpret_cast<const unsigned *>(S.bvh_nodes.data()), n_nodes, S.d.bvh_node16 != 0, S.d.n_all, order, level_off))
            return fail(RTMI_E_STATE, "the node array is not in parent-before-child order");
        return RTMI_OK;
    };
    int rc = build(0);
    if (rc) return rc;
    for (int step = 1; step < n_steps; ++step) {
        const SceneArrays a = arrays(step);
        rtmi_scene *none = nullptr;
        if ((rc = check_scene_args(a, &none)) != RTMI_OK) return rc;
        PackedScene P;
        GeomExtras X;
        pack_geometry_only(a, S.d.cull_t_lo, S.d.cull_t_hi, P, X);
        GeoVerdict V = judge_geometry(S.tree, S.d, S.host_kind, S.d.n_all, geom_was, SX.bounded, a.prim_geom, X, displaced);
        rebuilt_last = V.fits ? 0 : 1;
        if (!V.fits) { rebuilds++; if ((rc = build(step)) != RTMI_OK) return rc; continue; }
        if (n_nodes > 0) refit_host(reinterpret_cast<unsigned *>(S.bvh_nodes.data()), S.d.bvh_node16 != 0, V.leaf_box.data(), order);
        launches = 0;
        for (size_t h = 0; h + 1 < level_off.size(); ++h) launches += level_off[h + 1] > level_off[h];
        S.d.n_big = V.n_big;
        for (int k = 0; k < 16; ++k) S.d.big_idx[k] = k < V.n_big ? V.big_idx[k] : 0;
        displaced.swap(V.displaced); leaf_box.swap(V.leaf_box); displaced_n = V.n_displaced;
        SX = std::move(X);
        geom_was = a.prim_geom;
    }
    const int64_t bytes = (int64_t)(S.bvh_nodes.size() * sizeof(float));
    *out_bytes = bytes;
    if (out_nodes && bytes <= capacity) std::memcpy(out_nodes, S.bvh_nodes.data(), (size_t)bytes);
    const int32_t info[10] = {S.d.bvh_node16, S.d.bvh_root, S.d.grid_tall, S.d.grid_n, S.d.n_big, displaced_n, rebuilt_last, S.bvh_node_count, launches, rebuilds};
    std::memcpy(out_info, info, sizeof info);
    if (out_big) for (int k = 0; k < 16; ++k) out_big[k] = S.d.big_idx[k];
    if (out_cells) std::memcpy(out_cells, S.grid_cells.data(), (size_t)std::min<int64_t>(cells_capacity, (int64_t)S.grid_cells.size()) * sizeof(int));
    if (out_leaf_box) std::memcpy(out_leaf_box, leaf_box.data(), (size_t)S.d.n_all * 6 * sizeof(float));
    return RTMI_OK;
}
// ... and refit_half_outward against half_outward, the function it was ported from
RTMI_EXPORT int rtmi_test_refit_half(double x, int32_t up) { const float f = (float)x; unsigned u; std::memcpy(&u, &f, 4); return (int)refit_half_outward(u, up != 0); }

// test hook: the scene's node array as it lies in HBM (after the work queued on the context's stream); *out_bytes = its size, copied if it fits `capacity`
RTMI_EXPORT int rtmi_test_scene_nodes(rtmi_scene *s, void *buf, int64_t capacity, int64_t *out_bytes) {
    if (!out_bytes) return fail(RTMI_E_ARG, "out_bytes is NULL");
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    const int64_t bytes = (int64_t)s->bvh_node_count * (s->dev.bvh_node16 ? 32 : 64);
    *out_bytes = bytes;
    if (!buf || bytes > capacity || bytes == 0) return RTMI_OK;
    HIP_TRY(hipSetDevice(s->ctx->device));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    HIP_TRY(hipMemcpy(buf, s->dev.bvh_nodes, (size_t)bytes, hipMemcpyDeviceToHost));
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_scene_tree_info(const rtmi_scene *s, int32_t *out_info) {
    if (!scene_ok(const_cast<rtmi_scene *>(s))) return fail(RTMI_E_STATE, "invalid scene handle");
    if (!out_info) return fail(RTMI_E_ARG, "out_info is NULL");
    out_info[0] = s->bvh_node_count; out_info[1] = s->bvh_depth; out_info[2] = s->dev.grid_n; out_info[3] = s->dev.n_big;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_scene_device_bytes(rtmi_scene *s, int64_t *out_bytes) {
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    if (!out_bytes) return fail(RTMI_E_ARG, "out_bytes is NULL");
    *out_bytes = (int64_t)s->device_bytes;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_scene_destroy(rtmi_scene *s) {
    if (!s || s->magic != 0x52545343u) return fail(RTMI_E_STATE, "invalid scene handle");
    if (ctx_ok(s->ctx)) { (void)hipSetDevice(s->ctx->device); (void)hipStreamSynchronize(s->ctx->stream); }
    for (void *p : s->allocs) (void)hipFree(p);
    for (void *p : s->table_allocs) (void)hipFree(p);
    if (s->geo.d_order) (void)hipFree(s->geo.d_order);
    if (s->geo.d_leaf_box) (void)hipFree(s->geo.d_leaf_box);
    if (s->geo.ev0) (void)hipEventDestroy(s->geo.ev0);
    if (s->geo.ev1) (void)hipEventDestroy(s->geo.ev1);
    s->magic = 0;
    delete s;
    return RTMI_OK;
}

// ---- the hot path -------------------------------------------------------------------------------------
RTMI_EXPORT int32_t rtmi_local_tiles(int32_t nx, int32_t ny, int32_t first, int32_t stride) {
    if (nx <= 0 || ny <= 0 || first < 0 || stride <= 0) return 0;
    const int ntiles = tiles_x_of(nx) * tiles_y_of(ny);
    return first < ntiles ? (ntiles - first - 1) / stride + 1 : 0;
}

RTMI_EXPORT int rtmi_render_tiles_device(rtmi_scene *s, int32_t nx, int32_t ny, int32_t ns, int32_t depth, uint64_t seed, int32_t precision,
                                         int32_t tile_first, int32_t tile_stride, void *d_tiles_linear, void *d_out_counters, void *stream) {
    int rc = check_render_args(s, nx, ny, ns, depth, precision);
    if (rc) return rc;
    if (tile_first < 0 || tile_stride <= 0) return fail(RTMI_E_ARG, "tile_first must be >= 0 and tile_stride > 0");
    if (!d_tiles_linear) return fail(RTMI_E_ARG, "d_tiles_linear is NULL");
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = stream_of(s->ctx, stream);
    return with_real(precision, [&](auto r) { return render_tiles_impl<decltype(r)>(s, nx, ny, ns, depth, seed, tile_first, tile_stride, nullptr, d_tiles_linear, d_out_counters, st); });
}

RTMI_EXPORT int rtmi_assemble_device(rtmi_ctx *c, int32_t nx, int32_t ny, int32_t world, int32_t tiles_per_rank, const void *d_gathered,
                                     void *d_out_linear, void *d_out_rgb8, void *stream) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (nx <= 0 || ny <= 0 || world <= 0 || tiles_per_rank <= 0 || !d_gathered) return fail(RTMI_E_ARG, "bad assemble arguments");
    const int ntiles = tiles_x_of(nx) * tiles_y_of(ny);
    if ((long long)world * tiles_per_rank < ntiles) return fail(RTMI_E_ARG, "world*tiles_per_rank (%d*%d) does not cover %d tiles", world, tiles_per_rank, ntiles);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    const long long npx = (long long)nx * ny;
    // the 8-bit quantiser always runs in double on the double mean: both precisions share it
    hipLaunchKernelGGL((assemble_kernel<double>), dim3((unsigned)((npx + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       reinterpret_cast<const double *>(d_gathered), world, (size_t)tiles_per_rank * 192, tiles_x_of(nx), nx, ny,
                       reinterpret_cast<double *>(d_out_linear), reinterpret_cast<unsigned char *>(d_out_rgb8));
    HIP_TRY(hipGetLastError());
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_render_device(rtmi_scene *s, int32_t nx, int32_t ny, int32_t ns, int32_t depth, uint64_t seed, int32_t precision,
                                   void *d_out_linear, void *d_out_rgb8, void *d_out_counters, void *stream) {
    int rc = check_render_args(s, nx, ny, ns, depth, precision);
    if (rc) return rc;
    rtmi_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int ntiles = tiles_x_of(nx) * tiles_y_of(ny);
    rc = c->tiles.ensure((size_t)ntiles * 64 * 3 * sizeof(double));
    if (rc) return rc;
    rc = rtmi_render_tiles_device(s, nx, ny, ns, depth, seed, precision, 0, 1, c->tiles.p, d_out_counters, stream);
    if (rc) return rc;
    if (!d_out_linear && !d_out_rgb8) return RTMI_OK;
    return rtmi_assemble_device(c, nx, ny, 1, ntiles, c->tiles.p, d_out_linear, d_out_rgb8, stream);
}

RTMI_EXPORT int rtmi_render(rtmi_scene *s, int32_t nx, int32_t ny, int32_t ns, int32_t depth, uint64_t seed, int32_t precision,
                            int32_t x0, int32_t y0, int32_t x1, int32_t y1, double *out_linear, uint8_t *out_rgb8, uint64_t *out_counters) {
    int rc = check_render_args(s, nx, ny, ns, depth, precision);
    if (!rc) rc = check_region(nx, ny, x0, y0, x1, y1);
    if (rc) return rc;
    rtmi_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    // only the 8x8 tiles that intersect the region are rendered, and only the region's pixels in them are traced: both
    // counters describe exactly the region (a 16x8 spot check of a 1920x1080 frame costs 2 tiles, not 32400)
    const int w = x1 - x0, h = y1 - y0;
    const int tx0 = x0 / RTMI_TILE, ty0 = y0 / RTMI_TILE, tx1 = (x1 + RTMI_TILE - 1) / RTMI_TILE, ty1 = (y1 + RTMI_TILE - 1) / RTMI_TILE;
    const int wtx = tx1 - tx0, nwin = wtx * (ty1 - ty0);
    const size_t npx = (size_t)w * h;
    rc = c->tiles.ensure((size_t)nwin * 64 * 3 * sizeof(double));
    if (rc) return rc;
    HostIo io(c);
    FramePlanes d;
    rc = d.reserve(io, npx, false, true, false, out_linear, out_rgb8, nullptr, nullptr, out_counters);
    if (rc) return rc;
    const int rg[4] = {x0, y0, x1, y1};
    hipStream_t st = c->stream;
    rc = with_real(precision, [&](auto r) { return render_tiles_impl<decltype(r)>(s, nx, ny, ns, depth, seed, 0, 1, rg, c->tiles.p, d.cnt, st); });
    if (rc) return rc;
    hipLaunchKernelGGL((assemble_region_kernel<double>), dim3((unsigned)((npx + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       reinterpret_cast<const double *>(c->tiles.p), tx0, ty0, wtx, x0, y0, w, h, d.lin, d.q);
    return io.finish();
}

// ---- progressive rendering: a frame refined over calls ----------------------------------------------------------------
namespace {
// the checks of a progressive call; failing one leaves the context's frame as it was
int check_progressive_args(rtmi_scene *s, int nx, int ny, int s_first, int s_count, int depth, int precision) {
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    if (s_first < 0 || s_count <= 0) return fail(RTMI_E_ARG, "s_first must be >= 0 and s_count > 0 (got %d, %d)", s_first, s_count);
    if ((long long)s_first + s_count > INT32_MAX) return fail(RTMI_E_ARG, "s_first + s_count = %d + %d overflows int32", s_first, s_count);
    return check_render_args(s, nx, ny, s_count, depth, precision);
}

ProgKey progressive_key(const rtmi_scene *s, int nx, int ny, int depth, uint64_t seed, int precision, const int *rg) {
    ProgKey k;
    k.scene_serial = s->serial; k.scene_revision = s->revision; k.seed = seed;
    k.nx = nx; k.ny = ny; k.depth = depth; k.precision = precision;
    for (int i = 0; i < 4; ++i) k.rg[i] = rg[i];
    return k;
}

// s_first > 0 continues the context's frame: it must hold exactly s_first samples of the same key
int check_continuation(const rtmi_ctx *c, const ProgKey &k, int s_first) {
    if (s_first == 0) return RTMI_OK;
    const ProgFrame &f = c->prog;
    const ProgKey &a = f.key;
    if (f.k == 0) return fail(RTMI_E_STATE, "s_first = %d continues a progressive frame, but the context holds none (s_first = 0 starts one)", s_first);
    if (s_first != f.k) return fail(RTMI_E_STATE, "s_first = %d, but the context's progressive frame holds samples [0, %d)", s_first, f.k);
    if (k.scene_serial != a.scene_serial) return fail(RTMI_E_STATE, "the progressive frame was started with another scene");
    if (k.scene_revision != a.scene_revision) return fail(RTMI_E_STATE, "the scene was changed (rtmi_scene_set_*) after the progressive frame was started");
    if (k.nx != a.nx || k.ny != a.ny) return fail(RTMI_E_STATE, "nx x ny = %d x %d, the progressive frame is %d x %d", k.nx, k.ny, a.nx, a.ny);
    if (k.depth != a.depth) return fail(RTMI_E_STATE, "depth = %d, the progressive frame was started with %d", k.depth, a.depth);
    if (k.seed != a.seed) return fail(RTMI_E_STATE, "seed = %llu, the progressive frame was started with %llu", (unsigned long long)k.seed, (unsigned long long)a.seed);
    if (k.precision != a.precision) return fail(RTMI_E_STATE, "precision = %d, the progressive frame was started with %d", k.precision, a.precision);
    if (std::memcmp(k.rg, a.rg, sizeof k.rg))
        return fail(RTMI_E_STATE, "region [%d,%d)x[%d,%d), the progressive frame was started with [%d,%d)x[%d,%d)", k.rg[0], k.rg[2], k.rg[1], k.rg[3], a.rg[0], a.rg[2], a.rg[1], a.rg[3]);
    if (k.first != a.first || k.stride != a.stride)
        return fail(RTMI_E_STATE, "tile dealing (first %d, stride %d), the progressive frame was started with the dealing (first %d, stride %d)", k.first, k.stride, a.first, a.stride);
    return RTMI_OK;
}

// rtmi_render_progressive* cannot continue a frame in which a tile has retired: its image would not be render(ns = k)'s
int check_no_tile_retired(const rtmi_ctx *c, int s_first) {
    const ProgFrame &f = c->prog;
    if (s_first > 0 && f.k > 0 && f.adaptive && f.n_active < f.n_tiles)
        return fail(RTMI_E_STATE, "%d of the frame's %d tiles have retired (rtmi_render_adaptive): continue it with rtmi_render_adaptive, or start a new frame with s_first = 0",
                    f.n_tiles - f.n_active, f.n_tiles);
    return RTMI_OK;
}

// The frame's state resolved into the dense outputs of its region (device pointers, any may be null; none: nothing is launched), on `st`.
// per_tile: every local tile with its own sample count n_t (an adaptive frame); else the frame's k everywhere.
template <typename R>
hipError_t resolve_frame(const ProgFrame &f, const ProgKey &key, bool per_tile, double *d_lin, unsigned char *d_q, double *d_err, int *d_smp, hipStream_t st) {
    if (!d_lin && !d_q && !d_err && !d_smp) return hipSuccess;
    const int x0 = key.rg[0], y0 = key.rg[1], w = key.rg[2] - x0, h = key.rg[3] - y0;
    const int tx0 = x0 / RTMI_TILE, ty0 = y0 / RTMI_TILE, wtx = (key.rg[2] + RTMI_TILE - 1) / RTMI_TILE - tx0; // the local tiles of the region: this window, row-major
    const long long npx = (long long)w * h;
    hipLaunchKernelGGL((frame_resolve_kernel<R>), dim3((unsigned)((npx + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, reinterpret_cast<const R *>(f.sums.p),
                       reinterpret_cast<const double *>(f.m2.p), per_tile ? reinterpret_cast<const int *>(f.n_t.p) : (const int *)nullptr, f.k, tx0, ty0, wtx,
                       x0, y0, w, h, d_lin, d_q, d_err, d_smp);
    return hipGetLastError();
}

// Adds samples [s_first, s_first + s_count) to the context's frame (s_first = 0: a new frame), then resolves the state into the region's outputs
// (device pointers, any may be null) and copies the cumulative counters to d_cnt, all on `st`.
template <typename R>
int render_progressive_impl(rtmi_scene *s, const ProgKey &key, int s_first, int s_count, double *d_lin, unsigned char *d_q, double *d_err, void *d_cnt,
                            hipStream_t st) {
    ProgFrame &f = s->ctx->prog;
    int rc = render_passes<R>(s, key.nx, key.ny, s_first, s_first + s_count, key.depth, key.seed, 0, 1, key.rg, nullptr, nullptr, st, &f);
    if (rc) return rc;
    f.key = key;
    hipError_t e = resolve_frame<R>(f, key, false, d_lin, d_q, d_err, nullptr, st);
    if (e == hipSuccess && d_cnt) e = hipMemcpyAsync(d_cnt, f.counters.p, 2 * sizeof(u64), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) { f.k = 0; return fail(RTMI_E_DEVICE, "progressive resolve: %s", hipGetErrorString(e)); }
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_render_progressive_device(rtmi_scene *s, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                                               int32_t precision, void *d_out_linear, void *d_out_rgb8, void *d_out_stderr, void *d_out_counters, void *stream) {
    int rc = check_progressive_args(s, nx, ny, s_first, s_count, depth, precision);
    if (rc) return rc;
    const int whole[4] = {0, 0, nx, ny};
    const ProgKey key = progressive_key(s, nx, ny, depth, seed, precision, whole);
    rc = check_continuation(s->ctx, key, s_first);
    if (!rc) rc = check_no_tile_retired(s->ctx, s_first);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = stream_of(s->ctx, stream);
    double *lin = reinterpret_cast<double *>(d_out_linear), *err = reinterpret_cast<double *>(d_out_stderr);
    unsigned char *q = reinterpret_cast<unsigned char *>(d_out_rgb8);
    return with_real(precision, [&](auto r) { return render_progressive_impl<decltype(r)>(s, key, s_first, s_count, lin, q, err, d_out_counters, st); });
}

RTMI_EXPORT int rtmi_render_progressive(rtmi_scene *s, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                                        int32_t precision, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                                        double *out_linear, uint8_t *out_rgb8, double *out_stderr, uint64_t *out_counters) {
    int rc = check_progressive_args(s, nx, ny, s_first, s_count, depth, precision);
    if (!rc) rc = check_region(nx, ny, x0, y0, x1, y1);
    if (rc) return rc;
    const int rg[4] = {x0, y0, x1, y1};
    const ProgKey key = progressive_key(s, nx, ny, depth, seed, precision, rg);
    rtmi_ctx *c = s->ctx;
    rc = check_continuation(c, key, s_first);
    if (!rc) rc = check_no_tile_retired(c, s_first);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HostIo io(c);
    FramePlanes d;
    rc = d.reserve(io, (size_t)(x1 - x0) * (size_t)(y1 - y0), true, false, false, out_linear, out_rgb8, out_stderr, nullptr, nullptr);
    if (rc) return rc;
    hipStream_t st = c->stream;
    rc = with_real(precision, [&](auto r) { return render_progressive_impl<decltype(r)>(s, key, s_first, s_count, d.lin, d.q, d.err, nullptr, st); });
    if (rc) return rc;
    hipError_t e = io.download();
    if (e == hipSuccess && out_counters) e = hipMemcpy(out_counters, c->prog.counters.p, 2 * sizeof(u64), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { c->prog.k = 0; return fail(RTMI_E_DEVICE, "progressive render: %s", hipGetErrorString(e)); }
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_progressive_samples(rtmi_ctx *c, int32_t *samples) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (samples) *samples = c->prog.k;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_progressive_release(rtmi_ctx *c) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->prog.release();
    return RTMI_OK;
}

// ---- adaptive sampling: the frame's tiles stop taking samples once their noise is below eps -------------------------------------------------
namespace {
int check_adaptive_args(rtmi_scene *s, int nx, int ny, int s_first, int s_count, double eps, int depth, int precision) {
    int rc = check_progressive_args(s, nx, ny, s_first, s_count, depth, precision);
    if (rc) return rc;
    if (!(eps >= 0.0) || std::isinf(eps)) return fail(RTMI_E_ARG, "eps must be a finite number >= 0 (got %g)", eps);
    return RTMI_OK;
}

// Adds samples [s_first, s_first + s_count) to the active tiles of the context's frame, retires the tiles that pass eps, resolves the frame into
// the region's outputs (device pointers, any may be null), copies the cumulative counters to d_cnt and synchronises `st`: the host reads the
// length of the next active list.
template <typename R>
int render_adaptive_impl(rtmi_scene *s, const ProgKey &key, int s_first, int s_count, double eps, double *d_lin, unsigned char *d_q, double *d_err,
                         int *d_smp, void *d_cnt, hipStream_t st) {
    ProgFrame &f = s->ctx->prog;
    AdaptiveCall ad;
    ad.eps = eps; ad.k_before = s_first;
    int rc = render_passes<R>(s, key.nx, key.ny, s_first, s_first + s_count, key.depth, key.seed, 0, 1, key.rg, nullptr, nullptr, st, &f, &ad);
    if (rc) return rc;
    f.key = key;
    hipError_t e = resolve_frame<R>(f, key, true, d_lin, d_q, d_err, d_smp, st);
    if (e == hipSuccess && d_cnt) e = hipMemcpyAsync(d_cnt, f.counters.p, 2 * sizeof(u64), hipMemcpyDeviceToDevice, st);
    int meta[2] = {f.n_active, (int)f.active_pixels}; // both fit an int: check_render_args refuses frames above 2^30 pixels
    const bool traced = f.n_active > 0; // (the list this call started with: no trace, no compaction, meta unchanged)
    if (e == hipSuccess && traced) e = hipMemcpyAsync(meta, f.meta.p, sizeof meta, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { f.k = 0; return fail(RTMI_E_DEVICE, "adaptive resolve: %s", hipGetErrorString(e)); }
    f.pixel_samples += f.active_pixels * (long long)s_count; // the tiles active when the call started took its samples
    f.n_active = meta[0]; f.active_pixels = meta[1];
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_render_adaptive_device(rtmi_scene *s, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, double eps, int32_t depth,
                                            uint64_t seed, int32_t precision, void *d_out_linear, void *d_out_rgb8, void *d_out_stderr,
                                            void *d_out_samples, void *d_out_counters, void *stream) {
    int rc = check_adaptive_args(s, nx, ny, s_first, s_count, eps, depth, precision);
    if (rc) return rc;
    const int whole[4] = {0, 0, nx, ny};
    const ProgKey key = progressive_key(s, nx, ny, depth, seed, precision, whole);
    rc = check_continuation(s->ctx, key, s_first);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = stream_of(s->ctx, stream);
    double *lin = reinterpret_cast<double *>(d_out_linear), *err = reinterpret_cast<double *>(d_out_stderr);
    unsigned char *q = reinterpret_cast<unsigned char *>(d_out_rgb8);
    int *smp = reinterpret_cast<int *>(d_out_samples);
    return with_real(precision, [&](auto r) { return render_adaptive_impl<decltype(r)>(s, key, s_first, s_count, eps, lin, q, err, smp, d_out_counters, st); });
}

RTMI_EXPORT int rtmi_render_adaptive(rtmi_scene *s, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, double eps, int32_t depth, uint64_t seed,
                                     int32_t precision, int32_t x0, int32_t y0, int32_t x1, int32_t y1, double *out_linear, uint8_t *out_rgb8,
                                     double *out_stderr, int32_t *out_samples, uint64_t *out_counters) {
    int rc = check_adaptive_args(s, nx, ny, s_first, s_count, eps, depth, precision);
    if (!rc) rc = check_region(nx, ny, x0, y0, x1, y1);
    if (rc) return rc;
    const int rg[4] = {x0, y0, x1, y1};
    const ProgKey key = progressive_key(s, nx, ny, depth, seed, precision, rg);
    rtmi_ctx *c = s->ctx;
    rc = check_continuation(c, key, s_first);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HostIo io(c);
    FramePlanes d;
    rc = d.reserve(io, (size_t)(x1 - x0) * (size_t)(y1 - y0), true, false, true, out_linear, out_rgb8, out_stderr, out_samples, nullptr);
    if (rc) return rc;
    hipStream_t st = c->stream;
    rc = with_real(precision, [&](auto r) { return render_adaptive_impl<decltype(r)>(s, key, s_first, s_count, eps, d.lin, d.q, d.err, d.smp, nullptr, st); });
    if (rc) return rc;
    hipError_t e = io.download(); // (the stream is synchronised already)
    if (e == hipSuccess && out_counters) e = hipMemcpy(out_counters, c->prog.counters.p, 2 * sizeof(u64), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { c->prog.k = 0; return fail(RTMI_E_DEVICE, "adaptive render: %s", hipGetErrorString(e)); }
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_adaptive_status(rtmi_ctx *c, int32_t *active_tiles, int32_t *total_tiles, int64_t *pixel_samples) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    const ProgFrame &f = c->prog;
    const bool have = f.k > 0;
    if (active_tiles) *active_tiles = !have ? 0 : f.adaptive ? f.n_active : f.n_tiles;
    if (total_tiles) *total_tiles = have ? f.n_tiles : 0;
    if (pixel_samples) *pixel_samples = !have ? 0 : f.adaptive ? f.pixel_samples : f.valid_pixels * (long long)f.k;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_adaptive_active_tiles(rtmi_ctx *c, int32_t capacity, int32_t *out_tiles, int32_t *out_count) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    ProgFrame &f = c->prog;
    const int n = f.k <= 0 ? 0 : f.adaptive ? f.n_active : f.n_tiles;
    if (out_count) *out_count = n;
    if (!out_tiles || n == 0) return RTMI_OK;
    if (capacity < n) return fail(RTMI_E_ARG, "capacity = %d, the frame has %d active tiles", capacity, n);
    HIP_TRY(hipSetDevice(c->device));
    if (f.adaptive) { // the frame's own list, as the last compaction left it (every adaptive call ends with its stream synchronised)
        HIP_TRY(hipMemcpy(out_tiles, f.act_tiles[f.cur].p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    } else if (f.key.first != 0 || f.key.stride != 1) { // a uniform dealt frame (its region is the whole image): the dealing itself
        for (int i = 0; i < n; ++i) out_tiles[i] = f.key.first + i * f.key.stride;
    } else { // a uniform frame: every tile of the region, in tile order
        const int tx_n = tiles_x_of(f.key.nx), tx0 = f.key.rg[0] / RTMI_TILE, ty0 = f.key.rg[1] / RTMI_TILE;
        const int wtx = (f.key.rg[2] + RTMI_TILE - 1) / RTMI_TILE - tx0;
        for (int i = 0; i < n; ++i) out_tiles[i] = (ty0 + i / wtx) * tx_n + tx0 + i % wtx;
    }
    return RTMI_OK;
}

// ---- retiring tiles by a noise map the caller supplies (rtmi_adaptive_retire*) -------------------------------------------------------------------
namespace {
int check_retire_args(int nx, int ny, const void *noise, double eps) {
    if (nx <= 0 || ny <= 0) return fail(RTMI_E_ARG, "nx, ny must be > 0 (got %d %d)", nx, ny);
    if (!noise) return fail(RTMI_E_ARG, "noise is NULL");
    if (!(eps >= 0.0) || std::isinf(eps)) return fail(RTMI_E_ARG, "eps must be a finite number >= 0 (got %g)", eps);
    return RTMI_OK;
}

int check_retire_frame(const rtmi_ctx *c, int nx, int ny) {
    const ProgFrame &f = c->prog;
    if (f.k == 0) return fail(RTMI_E_STATE, "the context holds no progressive frame to retire tiles of (rtmi_render_adaptive or rtmi_render_progressive with s_first = 0 starts one)");
    if (nx != f.key.nx || ny != f.key.ny) return fail(RTMI_E_STATE, "nx x ny = %d x %d, the progressive frame is %d x %d", nx, ny, f.key.nx, f.key.ny);
    return RTMI_OK;
}

// Retires the active tiles of the context's frame whose pixels all pass d_noise <= eps (a device pointer to the whole-frame map) and synchronises
// `st`: the host reads the length of the next active list.  Nothing but the active list, its length and its pixel count changes.
int adaptive_retire_impl(rtmi_ctx *c, const double *d_noise, double eps, int32_t *out_retired, hipStream_t st) {
    ProgFrame &f = c->prog;
    const int nx = f.key.nx, ny = f.key.ny;
    const Region r = clip_region(f.key.rg, nx, ny);
    if (!f.adaptive) { // a uniform frame: the per-tile state as the first adaptive call builds it, every tile active with n_t = k
        int n_local = 0;
        int rc = ensure_tile_ids(c, nx, ny, f.key.first, f.key.stride, f.key.rg, st, &n_local); // (another render on the context may have rewritten its tile list)
        if (rc) return rc;
        if (n_local != f.n_tiles) return fail(RTMI_E_STATE, "progressive frame buffers do not match the frame"); // (unreachable: the key is the frame's own)
        rc = ensure_tile_state(f, reinterpret_cast<const int *>(c->tile_ids.p), n_local, f.k, tiles_x_of(nx), r, st, "adaptive retire");
        if (rc) { if (rc == RTMI_E_DEVICE) f.k = 0; return rc; } // (a failed launch drops the frame, a failed allocation does not)
    }
    if (out_retired) *out_retired = 0;
    if (f.n_active == 0) return RTMI_OK; // nothing to decide, nothing launched
    const int n = f.n_active;
    hipLaunchKernelGGL(adaptive_retire_kernel, dim3((unsigned)(((long long)n * 64 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, d_noise,
                       reinterpret_cast<const int *>(f.act_tiles[f.cur].p), n, tiles_x_of(nx), nx, r.x0, r.y0, r.x1, r.y1, eps, reinterpret_cast<int *>(f.keep.p));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = launch_compact(f, nullptr, n, -1, tiles_x_of(nx), r, st);
    int meta[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(meta, f.meta.p, sizeof meta, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { f.k = 0; return fail(RTMI_E_DEVICE, "adaptive retire: %s", hipGetErrorString(e)); }
    f.n_active = meta[0]; f.active_pixels = meta[1];
    if (out_retired) *out_retired = n - meta[0];
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_adaptive_retire_device(rtmi_ctx *c, int32_t nx, int32_t ny, const void *d_noise, double eps, int32_t *out_retired, void *stream) {
    int rc = check_retire_args(nx, ny, d_noise, eps);
    if (rc) return rc;
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    rc = check_retire_frame(c, nx, ny);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    return adaptive_retire_impl(c, reinterpret_cast<const double *>(d_noise), eps, out_retired, st);
}

RTMI_EXPORT int rtmi_adaptive_retire(rtmi_ctx *c, int32_t nx, int32_t ny, const double *noise, double eps, int32_t *out_retired) {
    int rc = check_retire_args(nx, ny, noise, eps);
    if (rc) return rc;
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    rc = check_retire_frame(c, nx, ny);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const ProgFrame &f = c->prog;
    if (f.adaptive && f.n_active == 0) { // nothing to decide: no upload, no launch
        if (out_retired) *out_retired = 0;
        return RTMI_OK;
    }
    HostIo io(c);
    double *d_noise;
    io.in(&d_noise, (size_t)nx * (size_t)ny, noise);
    rc = io.stage();
    if (rc) return rc;
    return adaptive_retire_impl(c, d_noise, eps, out_retired, c->stream);
}

// ---- one host process, several GPUs (the reference's host is ONE JVM: core.clj:100-108) ---------------------------------
RTMI_EXPORT int rtmi_scene_clone(rtmi_scene *src, rtmi_ctx *ctx, rtmi_scene **out_scene) {
    if (!scene_ok(src)) return fail(RTMI_E_STATE, "invalid scene handle");
    if (!ctx_ok(ctx)) return fail(RTMI_E_STATE, "invalid context handle");
    if (!out_scene) return fail(RTMI_E_ARG, "out_scene is NULL");
    DeviceGuard guard;
    const rtmi_scene::Args &A = src->args;
    rtmi_scene *s = nullptr;
    int rc = rtmi_scene_create_ex(ctx, src->n_prims, A.prim_kind.data(), A.prim_geom.data(), A.prim_mat.data(), src->n_mats, A.mat_kind.data(), A.mat_tex.data(),
                                  A.mat_param.data(), src->n_tex, A.tex_kind.data(), A.tex_param.data(), A.tex_child.data(), A.cam_kind, A.cam.data(),
                                  A.prim_flip.empty() ? nullptr : A.prim_flip.data(), A.prim_xform.empty() ? nullptr : A.prim_xform.data(),
                                  (int32_t)A.xform_kind.size(), A.xform_kind.empty() ? nullptr : A.xform_kind.data(),
                                  A.xform_param.empty() ? nullptr : A.xform_param.data(), &s);
    if (rc) return rc;
    if (!rc && !A.perlin_vec.empty()) rc = rtmi_scene_set_perlin(s, A.perlin_vec.data(), A.perm.data());
    if (!rc && !A.image_wh.empty()) rc = rtmi_scene_set_images(s, (int32_t)(A.image_wh.size() / 2), A.image_wh.data(), A.image_rgb.data());
    if (!rc && A.has_media_calls && A.media_mode == 2) rc = rtmi_scene_set_media_calls_narrowed(s, (int32_t)A.media_calls.size(), A.media_calls.data(), A.media_lo.data());
    else {
        if (!rc && A.has_media_calls) rc = rtmi_scene_set_media_calls(s, (int32_t)A.media_calls.size(), A.media_calls.data());
        if (!rc && A.media_mode) rc = rtmi_scene_set_media_mode(s, A.media_mode);
    }
    if (rc) { const std::string keep = g_err; rtmi_scene_destroy(s); g_err = keep; return rc; }
    *out_scene = s;
    return RTMI_OK;
}

namespace {
// RCCL, opened on first use: a single-GPU host never loads it.  (In a process that already maps an RCCL -- e.g. PyTorch's
// bundled one -- dlopen by soname returns that copy.)
struct Rccl {
    bool tried = false;
    void *h = nullptr;
    std::string err;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGather) Gather = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
std::mutex g_multi_mu;
Rccl g_rccl;
bool g_rccl_failed = false; // RCCL could not be opened / initialised / a gather failed once: later gathers use copies
std::map<std::vector<int>, std::vector<ncclComm_t>> g_comms; // one communicator set per device list (ncclCommInitAll), kept for the process

// Opens the first of `names` that dlopen accepts and binds the six entry points the gather needs.  On failure R.h stays null and
// R.err says why (dlerror() is read ONCE per failure: a second call returns NULL).
bool rccl_open(Rccl &R, const std::vector<std::string> &names) {
    std::string first_err;
    for (const std::string &name : names) {
        R.h = dlopen(name.c_str(), RTLD_NOW | RTLD_GLOBAL);
        if (R.h) break;
        const char *e = dlerror();
        if (first_err.empty()) first_err = std::string("dlopen(") + name + "): " + (e ? e : "not found");
    }
    if (!R.h) { R.err = first_err.empty() ? std::string("no library name given") : first_err; return false; }
    bool ok = true;
    auto sym = [&](const char *n) { void *p = dlsym(R.h, n); if (!p && ok) { ok = false; R.err = std::string("the RCCL library lacks ") + n; } return p; };
    R.CommInitAll = reinterpret_cast<decltype(R.CommInitAll)>(sym("ncclCommInitAll"));
    R.CommDestroy = reinterpret_cast<decltype(R.CommDestroy)>(sym("ncclCommDestroy"));
    R.GroupStart = reinterpret_cast<decltype(R.GroupStart)>(sym("ncclGroupStart"));
    R.GroupEnd = reinterpret_cast<decltype(R.GroupEnd)>(sym("ncclGroupEnd"));
    R.Gather = reinterpret_cast<decltype(R.Gather)>(sym("ncclGather"));
    R.GetErrorString = reinterpret_cast<decltype(R.GetErrorString)>(sym("ncclGetErrorString"));
    if (!ok) { dlclose(R.h); R.h = nullptr; }
    return ok;
}

std::vector<std::string> rccl_names() {
    if (const char *e = std::getenv("RTMI_RCCL_LIB")) return {std::string(e)}; // another build of RCCL, or a bogus name to rehearse the fallback
    return {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
}

bool rccl_load() {
    Rccl &R = g_rccl;
    if (R.tried) return R.h != nullptr;
    R.tried = true;
    return rccl_open(R, rccl_names());
}

int ensure_event(hipEvent_t *e) {
    if (!*e) HIP_TRY(hipEventCreate(e));
    return RTMI_OK;
}

// a communicator set that produced an error is not used again: destroy it and let later gathers copy
void rccl_give_up(const std::vector<int> &devs) {
    auto it = g_comms.find(devs);
    if (it != g_comms.end()) {
        for (ncclComm_t cm : it->second) if (cm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(cm);
        g_comms.erase(it);
    }
    g_rccl_failed = true;
}
} // namespace

// Can the RCCL library `soname` (NULL: the names the gather itself tries, or $RTMI_RCCL_LIB) be opened, and does it export the entry
// points the in-library gather binds?  No device is touched.
RTMI_EXPORT int rtmi_rccl_probe(const char *soname) {
    Rccl R;
    const bool ok = rccl_open(R, soname ? std::vector<std::string>{std::string(soname)} : rccl_names());
    if (!ok) return fail(RTMI_E_DEVICE, "%s", R.err.c_str());
    dlclose(R.h);
    return RTMI_OK;
}

namespace {
// How a multi-device call moves the replicas' records to replica 0's device, decided before anything is launched: RCCL whenever the replicas sit
// on distinct devices (n > 1); copies when they share a device (RCCL refuses duplicate devices in one communicator).  RTMI_MULTI_GATHER = "copy":
// never RCCL; "rccl": RCCL or an error -- no silent substitution -- and also for n = 1 (a one-rank communicator: the whole path -- dlopen,
// ncclCommInitAll, grouped in-place ncclGather -- on a one-GPU host).  The library owns its communicators: one set per device list, created on
// first use, kept for the process; without a usable RCCL the gather falls back to peer copies (same result, ordered with events), once and for all.
struct GatherPlan {
    bool use_rccl = false;
    std::vector<ncclComm_t> *comms = nullptr;
    std::vector<int> devs;
};

int plan_gather(int n, rtmi_scene *const *scenes, GatherPlan &g) {
    g.devs.resize((size_t)n);
    bool distinct = true;
    for (int r = 0; r < n; ++r) {
        g.devs[(size_t)r] = scenes[r]->ctx->device;
        for (int q = 0; q < r; ++q) distinct = distinct && g.devs[(size_t)q] != g.devs[(size_t)r];
    }
    const char *force = std::getenv("RTMI_MULTI_GATHER");
    const bool want_copy = force && !std::strcmp(force, "copy"), want_rccl = force && !std::strcmp(force, "rccl");
    if (want_rccl && !distinct) return fail(RTMI_E_ARG, "RTMI_MULTI_GATHER=rccl needs replicas on distinct devices (RCCL refuses one device twice in a communicator)");
    g.use_rccl = distinct && !want_copy && (want_rccl || (n > 1 && !g_rccl_failed));
    if (!g.use_rccl) return RTMI_OK;
    std::string why;
    if (!rccl_load()) why = g_rccl.err;
    else {
        auto it = g_comms.find(g.devs);
        if (it == g_comms.end()) {
            std::vector<ncclComm_t> cs((size_t)n);
            const ncclResult_t e = g_rccl.CommInitAll(cs.data(), n, g.devs.data());
            if (e != ncclSuccess) why = std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(e);
            else it = g_comms.emplace(g.devs, std::move(cs)).first;
        }
        if (why.empty()) g.comms = &it->second;
    }
    if (!why.empty()) {
        if (want_rccl) return fail(RTMI_E_DEVICE, "multi-device gather: %s", why.c_str());
        fprintf(stderr, "[rtmi] multi-device gather falls back to hipMemcpyPeerAsync: %s\n", why.c_str());
        g_rccl_failed = true;
        g.use_rccl = false;
    }
    return RTMI_OK;
}

// ONE gather of `words` 8-byte words per replica: recs[r] (on replica r's device, written on its context stream; with copies its ev_done is recorded
// behind the writes) -> gathered[r] on replica 0's device.  recs[0] = gathered: replica 0's record is in place.
int enqueue_gather(int n, rtmi_scene *const *scenes, const GatherPlan &g, const std::vector<char *> &recs, char *gathered, size_t words) {
    rtmi_ctx *c0 = scenes[0]->ctx;
    HIP_TRY(hipSetDevice(c0->device));
    int rc = ensure_event(&c0->ev_g0);
    if (!rc) rc = ensure_event(&c0->ev_g1);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c0->ev_g0, c0->stream));
    if (g.use_rccl) {
        ncclResult_t e = g_rccl.GroupStart();
        for (int r = 0; r < n && e == ncclSuccess; ++r) {
            (void)hipSetDevice(scenes[r]->ctx->device);
            e = g_rccl.Gather(recs[(size_t)r], r == 0 ? gathered : nullptr, words, ncclUint64, 0, (*g.comms)[(size_t)r], scenes[r]->ctx->stream);
        }
        const ncclResult_t e2 = g_rccl.GroupEnd();
        (void)hipSetDevice(c0->device);
        if (e == ncclSuccess) e = e2;
        if (e != ncclSuccess) { // this communicator set is not trusted again: later calls gather by copies
            const int code = fail(RTMI_E_DEVICE, "ncclGather: %s", g_rccl.GetErrorString(e));
            rccl_give_up(g.devs);
            return code;
        }
        c0->last_gather_path = RTMI_GATHER_RCCL;
    } else {
        bool peer = false;
        for (int r = 1; r < n; ++r) {
            rtmi_ctx *cr = scenes[r]->ctx;
            char *dst = gathered + (size_t)r * words * 8;
            HIP_TRY(hipStreamWaitEvent(c0->stream, cr->ev_done, 0));
            if (cr->device == c0->device) HIP_TRY(hipMemcpyAsync(dst, recs[(size_t)r], words * 8, hipMemcpyDeviceToDevice, c0->stream));
            else { peer = true; HIP_TRY(hipMemcpyPeerAsync(dst, c0->device, recs[(size_t)r], cr->device, words * 8, c0->stream)); }
            // replica r's NEXT render into its record waits for this copy (its stream is not otherwise ordered with replica 0's)
            if (cr->ev_consumed && cr->ev_consumed_device != c0->device) { (void)hipSetDevice(cr->ev_consumed_device); (void)hipEventDestroy(cr->ev_consumed); cr->ev_consumed = nullptr; HIP_TRY(hipSetDevice(c0->device)); }
            if (!cr->ev_consumed) { HIP_TRY(hipEventCreateWithFlags(&cr->ev_consumed, hipEventDisableTiming)); cr->ev_consumed_device = c0->device; }
            HIP_TRY(hipEventRecord(cr->ev_consumed, c0->stream));
            cr->consume_pending = true;
        }
        c0->last_gather_path = n == 1 ? RTMI_GATHER_NONE : (peer ? RTMI_GATHER_PEER_COPY : RTMI_GATHER_SAME_DEVICE);
    }
    HIP_TRY(hipEventRecord(c0->ev_g1, c0->stream));
    c0->have_gather = true;
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_render_multi_device(int32_t n, rtmi_scene *const *scenes, int32_t nx, int32_t ny, int32_t ns, int32_t depth, uint64_t seed,
                                         int32_t precision, void *d_out_linear, void *d_out_rgb8, void *d_out_counters) {
    if (n <= 0 || n > 64 || !scenes) return fail(RTMI_E_ARG, "n must be 1..64 and scenes non-NULL");
    for (int r = 0; r < n; ++r) {
        int rc = check_render_args(scenes[r], nx, ny, ns, depth, precision);
        if (rc) return rc;
        for (int q = 0; q < r; ++q)
            if (scenes[q]->ctx == scenes[r]->ctx) return fail(RTMI_E_ARG, "replicas %d and %d share a context (a context is not re-entrant: one per replica)", q, r);
        if (scenes[r]->n_prims != scenes[0]->n_prims) return fail(RTMI_E_ARG, "replica %d is not a clone of replica 0", r);
    }
    std::lock_guard<std::mutex> lock(g_multi_mu);
    DeviceGuard guard;
    GatherPlan plan;
    int rc = plan_gather(n, scenes, plan);
    if (rc) return rc;
    const int ntiles = tiles_x_of(nx) * tiles_y_of(ny);
    const int per = (ntiles + n - 1) / n;                  // every replica's record is padded to this many tiles
    const size_t rec = (size_t)per * 192 + 2;              // 8-byte words per record: tiles [per][64][3] doubles + the two metrics counters
    rtmi_ctx *c0 = scenes[0]->ctx;
    // From here on work is enqueued on the replicas' streams.  An error after the first launch must not return with kernels still in
    // flight on streams the caller believes idle (it may destroy the contexts next): bail() waits for every stream touched so far.
    int launched = 0;
    auto bail = [&](int code) {
        const std::string keep = g_err;
        for (int r = 0; r < launched; ++r) { (void)hipSetDevice(scenes[r]->ctx->device); (void)hipStreamSynchronize(scenes[r]->ctx->stream); }
        (void)hipSetDevice(c0->device); (void)hipStreamSynchronize(c0->stream);
        g_err = keep;
        return code;
    };
#define HIP_BAIL(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return bail(fail(RTMI_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_))); } while (0)
    // 1. every replica renders its tiles (r, r+n, ...) on its own device and stream, straight into its record
    HIP_TRY(hipSetDevice(c0->device));
    rc = c0->multi.ensure((size_t)n * rec * 8);
    if (rc) return rc;
    char *gathered = reinterpret_cast<char *>(c0->multi.p);
    std::vector<char *> recs((size_t)n);
    for (int r = 0; r < n; ++r) {
        rtmi_ctx *cr = scenes[r]->ctx;
        HIP_BAIL(hipSetDevice(cr->device));
        if (r == 0) recs[0] = gathered; // in place: replica 0's record is the first of the gathered buffer
        else { rc = cr->multi.ensure(rec * 8); if (rc) return bail(rc); recs[(size_t)r] = reinterpret_cast<char *>(cr->multi.p); }
        char *buf = recs[(size_t)r];
        if (cr->consume_pending) { // the previous frame's copy out of this record (on another replica 0's stream) must have read it
            HIP_BAIL(hipStreamWaitEvent(cr->stream, cr->ev_consumed, 0));
            cr->consume_pending = false;
        }
        launched = r + 1; // before the render: one that fails part-way is waited for
        rc = with_real(precision, [&](auto real) { return render_tiles_impl<decltype(real)>(scenes[r], nx, ny, ns, depth, seed, r, n, nullptr, buf, buf + (size_t)per * 192 * 8, cr->stream); });
        if (rc) return bail(rc);
        if (!plan.use_rccl && r > 0) { rc = ensure_event(&cr->ev_done); if (rc) return bail(rc); HIP_BAIL(hipEventRecord(cr->ev_done, cr->stream)); }
    }
    // 2. ONE gather to replica 0's device
    rc = enqueue_gather(n, scenes, plan, recs, gathered, rec);
    if (rc) return bail(rc);
    // 3. replica 0 un-tiles, quantises and sums the counters
    if (d_out_linear || d_out_rgb8) {
        const long long npx = (long long)nx * ny;
        hipLaunchKernelGGL((assemble_kernel<double>), dim3((unsigned)((npx + kBlock - 1) / kBlock)), dim3(kBlock), 0, c0->stream,
                           reinterpret_cast<const double *>(gathered), n, rec, tiles_x_of(nx), nx, ny,
                           reinterpret_cast<double *>(d_out_linear), reinterpret_cast<unsigned char *>(d_out_rgb8));
        HIP_BAIL(hipGetLastError());
    }
    if (d_out_counters) {
        hipLaunchKernelGGL(sum_counters_kernel, dim3(1), dim3(64), 0, c0->stream, reinterpret_cast<const u64 *>(gathered), n, rec, (size_t)per * 192,
                           reinterpret_cast<u64 *>(d_out_counters));
        HIP_BAIL(hipGetLastError());
    }
#undef HIP_BAIL
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_render_multi(int32_t n, rtmi_scene *const *scenes, int32_t nx, int32_t ny, int32_t ns, int32_t depth, uint64_t seed, int32_t precision,
                                  double *out_linear, uint8_t *out_rgb8, uint64_t *out_counters) {
    if (n <= 0 || !scenes || !scene_ok(scenes[0])) return fail(RTMI_E_ARG, "bad replica list");
    DeviceGuard guard;
    rtmi_ctx *c0 = scenes[0]->ctx;
    HIP_TRY(hipSetDevice(c0->device));
    HostIo io(c0);
    FramePlanes d;
    int rc = d.reserve(io, (size_t)nx * (size_t)ny, false, true, false, out_linear, out_rgb8, nullptr, nullptr, out_counters);
    if (rc) return rc;
    rc = rtmi_render_multi_device(n, scenes, nx, ny, ns, depth, seed, precision, d.lin, d.q, d.cnt);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c0->device));
    HIP_TRY(io.download()); // replica 0's stream is ordered after every replica's render through the gather
    for (int r = 1; r < n; ++r) { HIP_TRY(hipSetDevice(scenes[r]->ctx->device)); HIP_TRY(hipStreamSynchronize(scenes[r]->ctx->stream)); scenes[r]->ctx->consume_pending = false; }
    return RTMI_OK;
}

// ---- progressive and adaptive frames on dealt tiles: the per-device primitive, the assemble, the one-process driver -------------------------------
namespace {
// the checks of a dealt call that need no frame; failing one leaves every frame as it was
int check_adaptive_tiles_args(rtmi_scene *s, int nx, int ny, int s_first, int s_count, int retire, double eps, int depth, int precision, int tile_first,
                              int tile_stride) {
    if (tile_first < 0 || tile_stride <= 0) return fail(RTMI_E_ARG, "tile_first must be >= 0 and tile_stride > 0 (got %d, %d)", tile_first, tile_stride);
    if (s_first < 0 || s_count <= 0) return fail(RTMI_E_ARG, "s_first must be >= 0 and s_count > 0 (got %d, %d)", s_first, s_count);
    if (retire != 0 && retire != 1) return fail(RTMI_E_ARG, "retire must be 0 or 1 (got %d)", retire);
    if (retire && (!(eps >= 0.0) || std::isinf(eps))) return fail(RTMI_E_ARG, "eps must be a finite number >= 0 (got %g)", eps);
    return check_progressive_args(s, nx, ny, s_first, s_count, depth, precision);
}

ProgKey dealt_key(const rtmi_scene *s, int nx, int ny, int depth, uint64_t seed, int precision, int tile_first, int tile_stride) {
    const int whole[4] = {0, 0, nx, ny};
    ProgKey k = progressive_key(s, nx, ny, depth, seed, precision, whole);
    k.first = tile_first; k.stride = tile_stride;
    return k;
}

int check_dealt_continuation(const rtmi_ctx *c, const ProgKey &key, int s_first, int retire) {
    int rc = check_continuation(c, key, s_first);
    if (!rc && !retire) rc = check_no_tile_retired(c, s_first);
    return rc;
}

// Enqueues on `st`: samples [s_first, s_first + s_count) into the context's dealt frame (retire: rtmi_render_adaptive's two steps, else
// rtmi_render_progressive's one), the records of its local tiles into d_rec[n_slots][64][RTMI_PROG_REC] (n_slots >= the local tiles: the rest is
// zeroed), the cumulative counters into d_cnt, and the copy-back of the next active list's length.  Nothing waits: dealt_finish does.
template <typename R>
int dealt_launch(rtmi_scene *s, const ProgKey &key, int s_first, int s_count, int retire, double eps, double *d_rec, int n_slots, void *d_cnt,
                 hipStream_t st) {
    ProgFrame &f = s->ctx->prog;
    if (!f.meta_host && hipHostMalloc(reinterpret_cast<void **>(&f.meta_host), 2 * sizeof(int), hipHostMallocDefault) != hipSuccess) {
        f.meta_host = nullptr;
        (void)hipGetLastError();
        return fail(RTMI_E_NOMEM, "hipHostMalloc(%zu bytes) failed", 2 * sizeof(int));
    }
    f.meta_pending = false;
    AdaptiveCall ad;
    ad.eps = eps; ad.k_before = s_first;
    int rc = render_passes<R>(s, key.nx, key.ny, s_first, s_first + s_count, key.depth, key.seed, key.first, key.stride, key.rg, nullptr, nullptr, st, &f,
                              retire ? &ad : nullptr);
    if (rc) return rc;
    f.key = key;
    hipError_t e = hipSuccess;
    if (d_rec && n_slots > 0) {
        const long long npx = (long long)n_slots * 64;
        hipLaunchKernelGGL((progressive_record_kernel<R>), dim3((unsigned)((npx + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                           reinterpret_cast<const R *>(f.sums.p), reinterpret_cast<const double *>(f.m2.p),
                           f.adaptive ? reinterpret_cast<const int *>(f.n_t.p) : (const int *)nullptr, f.k, key.first, key.stride, tiles_x_of(key.nx), key.nx,
                           key.ny, f.n_tiles, n_slots, d_rec);
        e = hipGetLastError();
    }
    if (e == hipSuccess && d_cnt) e = hipMemcpyAsync(d_cnt, f.counters.p, 2 * sizeof(u64), hipMemcpyDeviceToDevice, st);
    const bool traced = retire && f.n_active > 0; // (the list this call started with: no trace, no compaction, meta unchanged)
    if (e == hipSuccess && traced) e = hipMemcpyAsync(f.meta_host, f.meta.p, 2 * sizeof(int), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) { f.k = 0; return fail(RTMI_E_DEVICE, "dealt resolve: %s", hipGetErrorString(e)); }
    f.meta_pending = traced;
    return RTMI_OK;
}

// Waits for `st` and brings the host's mirror of the frame's per-tile state up to date (render_adaptive_impl's last lines).
int dealt_finish(rtmi_ctx *c, int s_count, int retire, hipStream_t st) {
    ProgFrame &f = c->prog;
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) { f.k = 0; f.meta_pending = false; return fail(RTMI_E_DEVICE, "dealt render: %s", hipGetErrorString(e)); }
    if (retire) {
        f.pixel_samples += f.active_pixels * (long long)s_count; // the tiles active when the call started took its samples
        if (f.meta_pending) { f.n_active = f.meta_host[0]; f.active_pixels = f.meta_host[1]; }
    }
    f.meta_pending = false;
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_render_adaptive_tiles_device(rtmi_scene *s, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t retire, double eps,
                                                  int32_t depth, uint64_t seed, int32_t precision, int32_t tile_first, int32_t tile_stride,
                                                  void *d_tiles_rec, void *d_out_counters, void *stream) {
    int rc = check_adaptive_tiles_args(s, nx, ny, s_first, s_count, retire, eps, depth, precision, tile_first, tile_stride);
    if (rc) return rc;
    const ProgKey key = dealt_key(s, nx, ny, depth, seed, precision, tile_first, tile_stride);
    rc = check_dealt_continuation(s->ctx, key, s_first, retire);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = stream_of(s->ctx, stream);
    const int n_slots = rtmi_local_tiles(nx, ny, tile_first, tile_stride);
    double *rec = reinterpret_cast<double *>(d_tiles_rec);
    rc = with_real(precision, [&](auto r) { return dealt_launch<decltype(r)>(s, key, s_first, s_count, retire, eps, rec, n_slots, d_out_counters, st); });
    if (rc) return rc;
    return dealt_finish(s->ctx, s_count, retire, st);
}

RTMI_EXPORT int rtmi_assemble_progressive_device(rtmi_ctx *c, int32_t nx, int32_t ny, int32_t world, int32_t tiles_per_rank, const void *d_gathered_rec,
                                                 void *d_out_linear, void *d_out_rgb8, void *d_out_stderr, void *d_out_samples, void *stream) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (nx <= 0 || ny <= 0 || world <= 0 || tiles_per_rank <= 0 || !d_gathered_rec) return fail(RTMI_E_ARG, "bad assemble arguments");
    if ((long long)nx * ny > (1ll << 30)) return fail(RTMI_E_ARG, "frame too large");
    const int ntiles = tiles_x_of(nx) * tiles_y_of(ny);
    if ((long long)world * tiles_per_rank < ntiles) return fail(RTMI_E_ARG, "world*tiles_per_rank (%d*%d) does not cover %d tiles", world, tiles_per_rank, ntiles);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    const long long npx = (long long)nx * ny;
    hipLaunchKernelGGL(assemble_progressive_kernel, dim3((unsigned)((npx + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       reinterpret_cast<const double *>(d_gathered_rec), world, (size_t)tiles_per_rank * 64 * RTMI_PROG_REC, tiles_x_of(nx), nx, ny,
                       reinterpret_cast<double *>(d_out_linear), reinterpret_cast<unsigned char *>(d_out_rgb8), reinterpret_cast<double *>(d_out_stderr),
                       reinterpret_cast<int *>(d_out_samples));
    HIP_TRY(hipGetLastError());
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_render_multi_adaptive_device(int32_t n, rtmi_scene *const *scenes, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count,
                                                  int32_t retire, double eps, int32_t depth, uint64_t seed, int32_t precision, void *d_out_linear,
                                                  void *d_out_rgb8, void *d_out_stderr, void *d_out_samples, void *d_out_counters) {
    if (n <= 0 || n > 64 || !scenes) return fail(RTMI_E_ARG, "n must be 1..64 and scenes non-NULL");
    // every check of every replica comes before the first launch: a refusal leaves every frame as it was
    for (int r = 0; r < n; ++r) {
        int rc = check_adaptive_tiles_args(scenes[r], nx, ny, s_first, s_count, retire, eps, depth, precision, r, n);
        if (rc) return rc;
        for (int q = 0; q < r; ++q)
            if (scenes[q]->ctx == scenes[r]->ctx) return fail(RTMI_E_ARG, "replicas %d and %d share a context (a context is not re-entrant: one per replica)", q, r);
        if (scenes[r]->n_prims != scenes[0]->n_prims) return fail(RTMI_E_ARG, "replica %d is not a clone of replica 0", r);
    }
    std::vector<ProgKey> keys((size_t)n);
    for (int r = 0; r < n; ++r) {
        keys[(size_t)r] = dealt_key(scenes[r], nx, ny, depth, seed, precision, r, n);
        const int rc = check_dealt_continuation(scenes[r]->ctx, keys[(size_t)r], s_first, retire);
        if (rc) { const std::string why = g_err; return fail(rc, "replica %d: %s", r, why.c_str()); }
    }
    std::lock_guard<std::mutex> lock(g_multi_mu);
    DeviceGuard guard;
    GatherPlan plan;
    int rc = plan_gather(n, scenes, plan);
    if (rc) return rc;
    const int ntiles = tiles_x_of(nx) * tiles_y_of(ny);
    const int per = (ntiles + n - 1) / n;                             // every replica's record is padded to this many tiles
    const size_t tile_words = (size_t)per * 64 * RTMI_PROG_REC;       // doubles of a record's tiles
    const size_t rec = tile_words + 2;                                // 8-byte words per record: the tiles + the two metrics counters
    rtmi_ctx *c0 = scenes[0]->ctx;
    const int k_before0 = c0->prog.k;
    // An error once a frame has been touched drops the frame of EVERY replica (some hold the new samples, some do not: no continuation can be
    // right), and does not return with work in flight on streams the caller believes idle.
    int launched = 0;
    auto bail = [&](int code, bool drop) {
        const std::string keep = g_err;
        for (int r = 0; r < launched; ++r) { (void)hipSetDevice(scenes[r]->ctx->device); (void)hipStreamSynchronize(scenes[r]->ctx->stream); }
        (void)hipSetDevice(c0->device); (void)hipStreamSynchronize(c0->stream);
        if (drop) for (int r = 0; r < n; ++r) { scenes[r]->ctx->prog.k = 0; scenes[r]->ctx->prog.meta_pending = false; }
        g_err = keep;
        return code;
    };
#define HIP_BAIL(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return bail(fail(RTMI_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)), launched > 0); } while (0)
    // 1. every replica adds the samples to its dealt tiles (r, r + n, ...) on its own device and stream and resolves them straight into its record
    HIP_TRY(hipSetDevice(c0->device));
    rc = c0->multi.ensure((size_t)n * rec * 8);
    if (rc) return rc;
    char *gathered = reinterpret_cast<char *>(c0->multi.p);
    std::vector<char *> recs((size_t)n);
    for (int r = 0; r < n; ++r) {
        rtmi_ctx *cr = scenes[r]->ctx;
        HIP_BAIL(hipSetDevice(cr->device));
        if (r == 0) recs[0] = gathered; // in place: replica 0's record is the first of the gathered buffer
        else { rc = cr->multi.ensure(rec * 8); if (rc) return bail(rc, true); recs[(size_t)r] = reinterpret_cast<char *>(cr->multi.p); }
        char *buf = recs[(size_t)r];
        if (cr->consume_pending) { // the previous call's copy out of this record (on another replica 0's stream) must have read it
            HIP_BAIL(hipStreamWaitEvent(cr->stream, cr->ev_consumed, 0));
            cr->consume_pending = false;
        }
        rc = with_real(precision, [&](auto real) { return dealt_launch<decltype(real)>(scenes[r], keys[(size_t)r], s_first, s_count, retire, eps, reinterpret_cast<double *>(buf), per, buf + tile_words * 8, cr->stream); });
        // replica 0 refused before it touched its frame (the test hook, an allocation): nothing has changed anywhere
        if (rc) { launched = r + 1; return bail(rc, !(r == 0 && c0->prog.k == k_before0 && k_before0 > 0)); }
        launched = r + 1;
        if (!plan.use_rccl && r > 0) { rc = ensure_event(&cr->ev_done); if (rc) return bail(rc, true); HIP_BAIL(hipEventRecord(cr->ev_done, cr->stream)); }
    }
    // 2. ONE gather to replica 0's device (n = 1 without RTMI_MULTI_GATHER=rccl: nothing to move)
    rc = enqueue_gather(n, scenes, plan, recs, gathered, rec);
    if (rc) return bail(rc, true);
    // 3. replica 0 un-tiles, quantises and sums the counters
    HIP_BAIL(hipSetDevice(c0->device));
    if (d_out_linear || d_out_rgb8 || d_out_stderr || d_out_samples) {
        const long long npx = (long long)nx * ny;
        hipLaunchKernelGGL(assemble_progressive_kernel, dim3((unsigned)((npx + kBlock - 1) / kBlock)), dim3(kBlock), 0, c0->stream,
                           reinterpret_cast<const double *>(gathered), n, rec, tiles_x_of(nx), nx, ny, reinterpret_cast<double *>(d_out_linear),
                           reinterpret_cast<unsigned char *>(d_out_rgb8), reinterpret_cast<double *>(d_out_stderr), reinterpret_cast<int *>(d_out_samples));
        HIP_BAIL(hipGetLastError());
    }
    if (d_out_counters) {
        hipLaunchKernelGGL(sum_counters_kernel, dim3(1), dim3(64), 0, c0->stream, reinterpret_cast<const u64 *>(gathered), n, rec, tile_words,
                           reinterpret_cast<u64 *>(d_out_counters));
        HIP_BAIL(hipGetLastError());
    }
#undef HIP_BAIL
    // 4. the host's mirror of every replica's tile state; replica 0 last: its stream carries the gather and the assemble
    for (int r = n - 1; r >= 0; --r) {
        rtmi_ctx *cr = scenes[r]->ctx;
        if (hipSetDevice(cr->device) != hipSuccess) return bail(fail(RTMI_E_DEVICE, "hipSetDevice(%d) failed", cr->device), true);
        rc = dealt_finish(cr, s_count, retire, cr->stream);
        if (rc) return bail(rc, true);
    }
    for (int r = 1; r < n; ++r) scenes[r]->ctx->consume_pending = false; // replica 0's stream is idle: the copies out of the records are done
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_render_multi_adaptive(int32_t n, rtmi_scene *const *scenes, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t retire,
                                           double eps, int32_t depth, uint64_t seed, int32_t precision, double *out_linear, uint8_t *out_rgb8,
                                           double *out_stderr, int32_t *out_samples, uint64_t *out_counters) {
    if (n <= 0 || !scenes || !scene_ok(scenes[0])) return fail(RTMI_E_ARG, "bad replica list");
    if (nx <= 0 || ny <= 0 || (long long)nx * ny > (1ll << 30)) return fail(RTMI_E_ARG, "nx, ny must be > 0 and the frame at most 2^30 pixels (got %d %d)", nx, ny);
    DeviceGuard guard;
    rtmi_ctx *c0 = scenes[0]->ctx;
    HIP_TRY(hipSetDevice(c0->device));
    HostIo io(c0);
    FramePlanes d;
    int rc = d.reserve(io, (size_t)nx * (size_t)ny, true, true, true, out_linear, out_rgb8, out_stderr, out_samples, out_counters);
    if (rc) return rc;
    rc = rtmi_render_multi_adaptive_device(n, scenes, nx, ny, s_first, s_count, retire, eps, depth, seed, precision, d.lin, d.q, d.err, d.smp, d.cnt);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c0->device)); // (every replica's stream is synchronised)
    const hipError_t e = io.download();
    if (e != hipSuccess) {
        for (int r = 0; r < n; ++r) scenes[r]->ctx->prog.k = 0;
        return fail(RTMI_E_DEVICE, "multi-device adaptive render: %s", hipGetErrorString(e));
    }
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_last_gather_path(rtmi_ctx *c, int32_t *path) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (!c->have_gather) return fail(RTMI_E_STATE, "no multi-device render on this context yet");
    if (path) *path = c->last_gather_path;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_stream_idle(rtmi_ctx *c, int32_t *idle) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    HIP_TRY(hipSetDevice(c->device));
    const hipError_t e = hipStreamQuery(c->stream);
    if (e != hipSuccess && e != hipErrorNotReady) return fail(RTMI_E_DEVICE, "hipStreamQuery: %s", hipGetErrorString(e));
    if (idle) *idle = e == hipSuccess ? 1 : 0;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_last_record_reals(rtmi_ctx *c, int32_t *reals) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (!reals) return fail(RTMI_E_ARG, "reals is NULL");
    *reals = c->last_record_reals;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_last_passes(rtmi_ctx *c, int32_t *passes) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (passes) *passes = c->last_passes;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_last_accel(rtmi_ctx *c, int32_t *accel) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (c->last_accel < 0) return fail(RTMI_E_STATE, "no render on this context yet");
    if (accel) *accel = c->last_accel;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_last_gather_ms(rtmi_ctx *c, double *ms) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (!c->have_gather) return fail(RTMI_E_STATE, "no multi-device render on this context yet");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->ev_g1));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, c->ev_g0, c->ev_g1));
    if (ms) *ms = t;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_last_traversal_counters(rtmi_ctx *c, uint64_t *out_aabb_tests, uint64_t *out_prim_tests) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (!c->count_traversal) return fail(RTMI_E_STATE, "set option count_traversal = 1 before the render");
    if (!c->counters.p) return fail(RTMI_E_STATE, "no render on this context yet");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->last_stream ? c->last_stream : c->stream));
    u64 v[2] = {0, 0};
    HIP_TRY(hipMemcpy(v, reinterpret_cast<u64 *>(c->counters.p) + 3, sizeof v, hipMemcpyDeviceToHost));
    if (out_aabb_tests) *out_aabb_tests = v[0];
    if (out_prim_tests) *out_prim_tests = v[1];
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_last_trace_ms(rtmi_ctx *c, double *ms, int32_t *launches) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (!(c->flags & RTMI_FLAG_TIMING)) return fail(RTMI_E_STATE, "context was not created with RTMI_FLAG_TIMING");
    double total = 0.0, reduce = 0.0;
    for (int k = 0; k < c->events_used; ++k) {
        HIP_TRY(hipEventSynchronize(c->events[(size_t)k].second));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, c->events[(size_t)k].first, c->events[(size_t)k].second));
        total += t;
        if ((size_t)k < c->events_r.size()) {
            HIP_TRY(hipEventSynchronize(c->events_r[(size_t)k]));
            HIP_TRY(hipEventElapsedTime(&t, c->events[(size_t)k].second, c->events_r[(size_t)k]));
            reduce += t;
        }
    }
    if (ms) *ms = total;
    if (launches) *launches = c->events_used;
    c->last_reduce_ms = reduce; c->last_reduce_launches = c->events_used;
    c->events_used = 0; // the next render starts a new measurement window
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_last_reduce_ms(rtmi_ctx *c, double *ms, int32_t *launches) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (!(c->flags & RTMI_FLAG_TIMING)) return fail(RTMI_E_STATE, "context was not created with RTMI_FLAG_TIMING");
    if (ms) *ms = c->last_reduce_ms;
    if (launches) *launches = c->last_reduce_launches;
    return RTMI_OK;
}

// ---- probes ---------------------------------------------------------------------------------------------
namespace {
// What every probe of a scene checks first; then the scene's device is current.  n = 0 passes: the caller returns RTMI_OK at once.
int probe_begin(rtmi_scene *s, int precision, int n) {
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    if (precision != RTMI_F64 && precision != RTMI_F32) return fail(RTMI_E_ARG, "bad precision");
    if (n < 0) return fail(RTMI_E_ARG, "n < 0");
    if (n > 0) HIP_TRY(hipSetDevice(s->ctx->device));
    return RTMI_OK;
}
// A probe once its planes are named: the inputs go up, launch(stream, grid) starts the kernel over n items, the outputs come back.
template <typename Launch> int probe_run(HostIo &io, int n, Launch launch) {
    const int rc = io.stage();
    if (rc) return rc;
    launch(io.c->stream, dim3((unsigned)((n + kBlock - 1) / kBlock)));
    return io.finish();
}

// the two probe kernels that trace like a render: Family::kernel<R, VARIANT, EXT, MSEQ>() is the instantiation.  wave_level: the family has no
// LDS-staged scan (no workgroup barriers), so its only dynamic LDS is the traversal's stack columns
struct ProbeHit {
    static constexpr bool wave_level = false;
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return probe_hit_kernel<R, V, EXT, MSEQ>; }
};
struct ProbePaths {
    static constexpr bool wave_level = false;
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return probe_paths_kernel<R, V, EXT, MSEQ>; }
};

// The probe instantiation the scene and the context select (precision x mixed kinds x media_seq x accel / scan_variant) and its dynamic LDS:
// launch(kernel, lds_bytes, prims_per_tile, n_ptiles).  Mixed-kind scenes have FP64 kernels only (the entries refuse RTMI_F32 for them).
// force_flat: answer a request for the tree with the flat scan (the queries' use of option "flat_below"; the scans find the same hits).
template <typename Family, typename R, typename Launch> void with_probe_kernel(const rtmi_scene *s, Launch launch, bool force_flat = false) {
    const rtmi_ctx *c = s->ctx;
    int ppt, npt;
    size_t lds;
    lds_plan(c, s->dev.n_static, sizeof(R), &ppt, &npt, &lds);
    if (Family::wave_level) lds = 64;
    const size_t bvh_lds = (size_t)RTMI_BVH_STACK * kBlock * sizeof(int) + 16; // the traversal's stack columns
    const bool bvh = c->accel == RTMI_ACCEL_BVH && !force_flat;
    if constexpr (std::is_same<R, double>::value) {
        if (s->dev.has_ext) { // (operands in the order the kernels were always instantiated in: the device code's inlining follows that order)
            const int seq = s->dev.media_seq;
            if (bvh) launch(seq != 2 ? (seq ? Family::template kernel<double, SCAN_BVH, true, 1>() : Family::template kernel<double, SCAN_BVH, true>())
                                     : Family::template kernel<double, SCAN_BVH, true, 2>(), bvh_lds, ppt, npt);
            else launch(seq != 2 ? (seq ? Family::template kernel<double, SCAN_SGPR_CULL, true, 1>() : Family::template kernel<double, SCAN_SGPR_CULL, true>())
                                 : Family::template kernel<double, SCAN_SGPR_CULL, true, 2>(), (size_t)64, ppt, npt);
            return;
        }
    }
    switch (bvh ? SCAN_BVH : c->scan_variant) {
    case SCAN_BVH: launch(Family::template kernel<R, SCAN_BVH>(), std::max(lds, bvh_lds), ppt, npt); break;
    case SCAN_SGPR_CULL: launch(Family::template kernel<R, SCAN_SGPR_CULL>(), lds, ppt, npt); break;
    case SCAN_SGPR: launch(Family::template kernel<R, SCAN_SGPR>(), lds, ppt, npt); break;
    case SCAN_LDS_PIPE: launch(Family::template kernel<R, SCAN_LDS_PIPE>(), lds, ppt, npt); break;
    default: launch(Family::template kernel<R, SCAN_LDS_LITERAL>(), lds, ppt, npt);
    }
}
} // namespace

RTMI_EXPORT int rtmi_probe_hit(rtmi_scene *s, int32_t precision, int32_t n, const double *rays, double t_min, double t_max, double *out) {
    const int rc = probe_begin(s, precision, n);
    if (rc || n == 0) return rc;
    if (!rays || !out) return fail(RTMI_E_ARG, "NULL array");
    if (precision == RTMI_F32 && s->dev.has_ext) return fail(RTMI_E_UNSUPPORTED, "rectangles / triangles / instances are FP64 only");
    HostIo io(s->ctx);
    double *d_rays, *d_out;
    io.in(&d_rays, (size_t)n * 7, rays); io.out(&d_out, (size_t)n * 11, out);
    return probe_run(io, n, [&](hipStream_t st, dim3 grid) {
        auto run = [&](auto kern, size_t lds, int ppt, int npt) { hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, st, s->d_dev, ppt, npt, n, d_rays, t_min, t_max, d_out); };
        with_real(precision, [&](auto r) { with_probe_kernel<ProbeHit, decltype(r)>(s, run); });
    });
}

RTMI_EXPORT int rtmi_probe_paths(rtmi_scene *s, int32_t precision, int32_t n, const double *rays, const uint64_t *keys, uint64_t ctr0, int32_t depth,
                                 double *out_rgb, uint64_t *out_nseg, double *log, int32_t max_seg, int32_t *out_nlog) {
    const int rc = probe_begin(s, precision, n);
    if (rc || n == 0) return rc;
    if (!rays || !keys || !out_rgb) return fail(RTMI_E_ARG, "NULL array");
    if (log && max_seg <= 0) return fail(RTMI_E_ARG, "log given but max_seg <= 0");
    if (precision == RTMI_F32 && s->dev.has_ext) return fail(RTMI_E_UNSUPPORTED, "rectangles / triangles / instances are FP64 only");
    HostIo io(s->ctx);
    double *d_rays, *d_rgb, *d_log;
    u64 *d_keys, *d_nseg;
    int *d_nlog;
    const size_t log_words = log ? (size_t)n * max_seg * RTMI_SEG_REC : 0;
    io.in(&d_rays, (size_t)n * 7, rays); io.in(&d_keys, (size_t)n, keys); io.out(&d_rgb, (size_t)n * 3, out_rgb);
    io.work(&d_nseg, (size_t)n, out_nseg); io.work(&d_nlog, (size_t)n, out_nlog); io.out(&d_log, log_words, log);
    return probe_run(io, n, [&](hipStream_t st, dim3 grid) {
        if (d_log && hipMemset(d_log, 0, log_words * sizeof(double)) != hipSuccess) return; // (probe_run reports the error)
        auto run = [&](auto kern, size_t lds, int ppt, int npt) {
            hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, st, s->d_dev, ppt, npt, n, d_rays, d_keys, (u64)ctr0, depth, d_rgb, d_nseg, d_log, max_seg, d_nlog);
        };
        with_real(precision, [&](auto r) { with_probe_kernel<ProbePaths, decltype(r)>(s, run); });
    });
}

RTMI_EXPORT int rtmi_probe_camera(rtmi_scene *s, int32_t precision, int32_t n, const double *uv, const uint64_t *keys, double *out) {
    const int rc = probe_begin(s, precision, n);
    if (rc || n == 0) return rc;
    if (!uv || !keys || !out) return fail(RTMI_E_ARG, "NULL array");
    HostIo io(s->ctx);
    double *d_uv, *d_out;
    u64 *d_keys;
    io.in(&d_uv, (size_t)n * 2, uv); io.in(&d_keys, (size_t)n, keys); io.out(&d_out, (size_t)n * 8, out);
    return probe_run(io, n, [&](hipStream_t st, dim3 grid) {
        with_real(precision, [&](auto r) { hipLaunchKernelGGL((probe_camera_kernel<decltype(r)>), grid, dim3(kBlock), 0, st, s->d_dev, n, d_uv, d_keys, d_out); });
    });
}

RTMI_EXPORT int rtmi_probe_texture(rtmi_scene *s, int32_t precision, int32_t tex, int32_t n, const double *uvp, double *out) {
    const int rc = probe_begin(s, precision, n);
    if (rc || n == 0) return rc;
    if (!uvp || !out) return fail(RTMI_E_ARG, "NULL array");
    if (tex < 0 || tex >= s->n_tex) return fail(RTMI_E_ARG, "texture index %d out of range", tex);
    if (s->dev.has_ext && precision != RTMI_F64) return fail(RTMI_E_UNSUPPORTED, "procedural / image textures are FP64 only");
    HostIo io(s->ctx);
    double *d_in, *d_out;
    io.in(&d_in, (size_t)n * 5, uvp); io.out(&d_out, (size_t)n * 3, out);
    return probe_run(io, n, [&](hipStream_t st, dim3 grid) {
        if (s->dev.has_ext) hipLaunchKernelGGL((probe_texture_kernel<double, true>), grid, dim3(kBlock), 0, st, s->d_dev, tex, n, d_in, d_out);
        else if (precision == RTMI_F64) hipLaunchKernelGGL((probe_texture_kernel<double>), grid, dim3(kBlock), 0, st, s->d_dev, tex, n, d_in, d_out);
        else hipLaunchKernelGGL((probe_texture_kernel<float>), grid, dim3(kBlock), 0, st, s->d_dev, tex, n, d_in, d_out);
    });
}

RTMI_EXPORT int rtmi_probe_scatter(rtmi_scene *s, int32_t precision, int32_t mat, int32_t n, const double *rays, const double *hits,
                                   const uint64_t *keys, double *out) {
    const int rc = probe_begin(s, precision, n);
    if (rc || n == 0) return rc;
    if (!rays || !hits || !keys || !out) return fail(RTMI_E_ARG, "NULL array");
    if (mat < 0 || mat >= s->n_mats) return fail(RTMI_E_ARG, "material index %d out of range", mat);
    if (s->dev.has_ext && precision != RTMI_F64) return fail(RTMI_E_UNSUPPORTED, "procedural / image textures are FP64 only");
    HostIo io(s->ctx);
    double *d_rays, *d_hits, *d_out;
    u64 *d_keys;
    io.in(&d_rays, (size_t)n * 7, rays); io.in(&d_hits, (size_t)n * 8, hits); io.in(&d_keys, (size_t)n, keys); io.out(&d_out, (size_t)n * 9, out);
    return probe_run(io, n, [&](hipStream_t st, dim3 grid) {
        if (s->dev.has_ext) hipLaunchKernelGGL((probe_scatter_kernel<double, true>), grid, dim3(kBlock), 0, st, s->d_dev, mat, n, d_rays, d_hits, d_keys, d_out);
        else if (precision == RTMI_F64) hipLaunchKernelGGL((probe_scatter_kernel<double>), grid, dim3(kBlock), 0, st, s->d_dev, mat, n, d_rays, d_hits, d_keys, d_out);
        else hipLaunchKernelGGL((probe_scatter_kernel<float>), grid, dim3(kBlock), 0, st, s->d_dev, mat, n, d_rays, d_hits, d_keys, d_out);
    });
}

RTMI_EXPORT int rtmi_probe_rng(rtmi_ctx *c, int32_t precision, uint64_t key, uint64_t d0, int32_t n, uint64_t *out_bits, double *out_real) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (precision != RTMI_F64 && precision != RTMI_F32) return fail(RTMI_E_ARG, "bad precision");
    if (n <= 0 || !out_bits || !out_real) return fail(RTMI_E_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HostIo io(c);
    u64 *d_bits;
    double *d_real;
    io.out(&d_bits, (size_t)n, out_bits); io.out(&d_real, (size_t)n, out_real);
    return probe_run(io, n, [&](hipStream_t st, dim3 grid) {
        with_real(precision, [&](auto r) { hipLaunchKernelGGL((probe_rng_kernel<decltype(r)>), grid, dim3(kBlock), 0, st, (u64)key, (u64)d0, n, d_bits, d_real); });
    });
}

// the path's own FP64 helpers (rtmi_device.h): square root with the wave-uniform fast path, the table-driven atan2 / asin and the uv
// formula of get-sphere-uv, the per-ray reciprocal of the sphere roots, division by a constant
__global__ void probe_math_kernel(int n, const double *abc, double tmin, double tmax, int n_slots, double *out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double a = abc[3 * k], b = abc[3 * k + 1], c = abc[3 * k + 2];
    double o[RTMI_PROBE_MATH_SLOTS];
    o[0] = rt_sqrt(a);
    const TrigTable K = trig_table();
    o[1] = rt_atan2(a, b, K);
    o[2] = rt_asin(a, K);
    Real<double>::sphere_uv(a, b, c, &o[3], &o[4]);
    const Quot<double> q = make_quot<double>(b, tmin, tmax);
    o[5] = q(a);
    o[6] = div_const(a, K[29], K[27]);
    o[7] = (double)q.fast;
    o[8] = (double)float_above(c); // the traversal's float bound of the closest hit so far: a float >= c, within two ulps
    o[9] = rt_log_unit(a);         // ConstantMedium's free-flight log of a draw in [0, 1)
    const bool fast = rcp_in_range(b) && tmin >= 0x1p-300 && tmax <= 0x1p200; // a rectangle's t = a / b by the refined reciprocal of a signed divisor (ext_box_faces, scan_small_ext)
    o[10] = div_by(a, refined_rcp(b), fast);
    o[11] = (double)fast;
    for (int j = 0; j < n_slots; ++j) out[(size_t)k * n_slots + j] = o[j];
}

RTMI_EXPORT int rtmi_probe_arith(rtmi_ctx *c, int32_t n, const double *abc, double *out) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (n <= 0 || !abc || !out) return fail(RTMI_E_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HostIo io(c);
    double *d_in, *d_out;
    io.in(&d_in, (size_t)n * 3, abc); io.out(&d_out, (size_t)n * 3, out);
    return probe_run(io, n, [&](hipStream_t st, dim3 grid) { hipLaunchKernelGGL(probe_arith_kernel, grid, dim3(kBlock), 0, st, n, d_in, d_out); });
}

// n_slots values per triple (1 .. RTMI_PROBE_MATH_SLOTS): the caller states how many its buffer holds per triple
RTMI_EXPORT int rtmi_probe_math2(rtmi_ctx *c, int32_t n, const double *abc, double tmin, double tmax, int32_t n_slots, double *out) {
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (n <= 0 || !abc || !out) return fail(RTMI_E_ARG, "bad arguments");
    if (n_slots < 1 || n_slots > RTMI_PROBE_MATH_SLOTS) return fail(RTMI_E_ARG, "n_slots must be 1..%d", RTMI_PROBE_MATH_SLOTS);
    HIP_TRY(hipSetDevice(c->device));
    HostIo io(c);
    double *d_in, *d_out;
    io.in(&d_in, (size_t)n * 3, abc); io.out(&d_out, (size_t)n * (size_t)n_slots, out);
    return probe_run(io, n, [&](hipStream_t st, dim3 grid) { hipLaunchKernelGGL(probe_math_kernel, grid, dim3(kBlock), 0, st, n, d_in, tmin, tmax, (int)n_slots, d_out); });
}
// the entry as first published: EIGHT values per triple (version 203 wrote nine into the same signature; hosts built against either header get eight again)
RTMI_EXPORT int rtmi_probe_math(rtmi_ctx *c, int32_t n, const double *abc, double tmin, double tmax, double *out) {
    return rtmi_probe_math2(c, n, abc, tmin, tmax, 8, out);
}

// ---- first-hit feature buffers (rtmi_render_features*) -----------------------------------------------------------------------------------------
namespace {
// feature_kernel's instantiations are chosen where the probe kernels' are (with_probe_kernel); the LDS-staged scans (scan_variant 0 / 1) need
// workgroup barriers and are answered with the scalar-cache scan, which finds the same hit
struct FeaturePass {
    static constexpr bool wave_level = true;
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return feature_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT, MSEQ>; }
};

int check_feature_args(rtmi_scene *s, int nx, int ny, int na, int precision) {
    if (na <= 0) return fail(RTMI_E_ARG, "na must be > 0 (got %d)", na);
    if (nx <= 0 || ny <= 0) return fail(RTMI_E_ARG, "nx, ny must be > 0 (got %d %d)", nx, ny);
    return check_render_args(s, nx, ny, na, 0, precision);
}

// the region rg = {x0, y0, x1, y1} of the frame's features into d_out[y1 - y0][x1 - x0][8], the counters into d_cnt[2]; all on `st`
template <typename R>
int render_features_impl(rtmi_scene *s, int nx, int ny, int na, uint64_t seed, const int *rg, double *d_out, u64 *d_cnt, hipStream_t st) {
    FeatureParams fp;
    fp.nx = nx; fp.ny = ny; fp.na = na; fp.seed = seed;
    fp.tx0 = rg[0] / RTMI_TILE; fp.ty0 = rg[1] / RTMI_TILE;
    fp.wtx = (rg[2] + RTMI_TILE - 1) / RTMI_TILE - fp.tx0;
    fp.n_tiles = fp.wtx * ((rg[3] + RTMI_TILE - 1) / RTMI_TILE - fp.ty0);
    fp.rx0 = rg[0]; fp.ry0 = rg[1]; fp.rx1 = rg[2]; fp.ry1 = rg[3];
    fp.out = d_out; fp.counters = d_cnt;
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 2 * sizeof(u64), st));
    const unsigned grid = (unsigned)((fp.n_tiles + kBlock / 64 - 1) / (kBlock / 64));
    with_probe_kernel<FeaturePass, R>(s, [&](auto kern, size_t lds, int, int) { hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, st, s->d_dev, fp); });
    HIP_TRY(hipGetLastError());
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_render_features_device(rtmi_scene *s, int32_t nx, int32_t ny, int32_t na, uint64_t seed, int32_t precision,
                                            void *d_out_features, void *d_out_counters, void *stream) {
    int rc = check_feature_args(s, nx, ny, na, precision);
    if (rc) return rc;
    if (!d_out_features) return fail(RTMI_E_ARG, "d_out_features is NULL");
    rtmi_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    if (!d_out_counters) {
        rc = c->feat_cnt.ensure(2 * sizeof(u64));
        if (rc) return rc;
        d_out_counters = c->feat_cnt.p;
    }
    const int whole[4] = {0, 0, nx, ny};
    return with_real(precision, [&](auto r) { return render_features_impl<decltype(r)>(s, nx, ny, na, seed, whole, reinterpret_cast<double *>(d_out_features), reinterpret_cast<u64 *>(d_out_counters), st); });
}

RTMI_EXPORT int rtmi_render_features(rtmi_scene *s, int32_t nx, int32_t ny, int32_t na, uint64_t seed, int32_t precision,
                                     int32_t x0, int32_t y0, int32_t x1, int32_t y1, double *out_features, uint64_t *out_counters) {
    int rc = check_feature_args(s, nx, ny, na, precision);
    if (!rc) rc = check_region(nx, ny, x0, y0, x1, y1);
    if (rc) return rc;
    if (!out_features) return fail(RTMI_E_ARG, "out_features is NULL");
    rtmi_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    HostIo io(c);
    double *d_out;
    u64 *d_cnt;
    io.out(&d_out, (size_t)(x1 - x0) * (size_t)(y1 - y0) * 8, out_features); io.work(&d_cnt, 2, out_counters);
    rc = io.reserve();
    if (rc) return rc;
    const int rg[4] = {x0, y0, x1, y1};
    hipStream_t st = c->stream;
    rc = with_real(precision, [&](auto r) { return render_features_impl<decltype(r)>(s, nx, ny, na, seed, rg, d_out, d_cnt, st); });
    return rc ? rc : io.finish();
}

// ---- edge-aware denoiser (rtmi_denoise*) ---------------------------------------------------------------------------------------------------------
namespace {
// the argument checks of both entries, before the handle is looked at: they need no device
int check_denoise_args(int nx, int ny, const void *lin, int iterations, double sigma_c, double sigma_n, double sigma_a, double sigma_d) {
    if (nx <= 0 || ny <= 0) return fail(RTMI_E_ARG, "nx, ny must be > 0 (got %d %d)", nx, ny);
    if ((long long)nx * ny > (1ll << 30)) return fail(RTMI_E_ARG, "frame too large");
    if (iterations < 0 || iterations > 8) return fail(RTMI_E_ARG, "iterations must be 0..8 (got %d)", iterations);
    const double sg[4] = {sigma_c, sigma_n, sigma_a, sigma_d};
    for (int k = 0; k < 4; ++k)
        if (!(sg[k] >= 0.0)) return fail(RTMI_E_ARG, "sigma_%c must be >= 0 and not NaN (got %g)", "cnad"[k], sg[k]);
    if (!lin) return fail(RTMI_E_ARG, "linear_in is NULL");
    return RTMI_OK;
}

int denoise_impl(rtmi_ctx *c, int nx, int ny, const double *d_lin, const double *d_se, const double *d_feat, int iterations, double sigma_c,
                 double sigma_n, double sigma_a, double sigma_d, double *d_out_lin, unsigned char *d_out_q, double *d_out_se, hipStream_t st) {
    const size_t n = (size_t)nx * (size_t)ny;
    int rc = c->dn_planes.ensure((2 * kDnState + (d_feat ? kDnFeat : 0)) * n * sizeof(double));
    if (rc) return rc;
    double *state[2] = {reinterpret_cast<double *>(c->dn_planes.p), reinterpret_cast<double *>(c->dn_planes.p) + kDnState * n};
    double *fplanes = d_feat ? state[1] + kDnState * n : nullptr;
    const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(denoise_load_kernel, dim3(blocks), dim3(kBlock), 0, st, d_lin, d_se, d_feat, n, state[0], fplanes);
    HIP_TRY(hipGetLastError());
    const int use_c = d_se && sigma_c > 0.0, use_n = d_feat && sigma_n > 0.0, use_a = d_feat && sigma_a > 0.0, use_d = d_feat && sigma_d > 0.0;
    int cur = 0;
    for (int i = 0; i < iterations; ++i, cur = 1 - cur) {
        hipLaunchKernelGGL(denoise_pass_kernel, dim3((unsigned)((nx + 63) / 64), (unsigned)((ny + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, st,
                           state[cur], state[1 - cur], fplanes, nx, ny, 1 << i, use_c, use_n, use_a, use_d, sigma_c * sigma_c, sigma_n * sigma_n,
                           sigma_a * sigma_a, sigma_d * sigma_d);
        HIP_TRY(hipGetLastError());
    }
    if (d_out_lin || d_out_q || d_out_se) {
        hipLaunchKernelGGL(denoise_store_kernel, dim3(blocks), dim3(kBlock), 0, st, state[cur], n, iterations == 0 ? d_se : (const double *)nullptr, d_out_lin,
                           d_out_q, d_out_se);
        HIP_TRY(hipGetLastError());
    }
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_denoise_device(rtmi_ctx *c, int32_t nx, int32_t ny, const void *d_linear_in, const void *d_stderr_in, const void *d_features_in,
                                    int32_t iterations, double sigma_c, double sigma_n, double sigma_a, double sigma_d,
                                    void *d_out_linear, void *d_out_rgb8, void *d_out_stderr, void *stream) {
    int rc = check_denoise_args(nx, ny, d_linear_in, iterations, sigma_c, sigma_n, sigma_a, sigma_d);
    if (rc) return rc;
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    return denoise_impl(c, nx, ny, reinterpret_cast<const double *>(d_linear_in), reinterpret_cast<const double *>(d_stderr_in),
                        reinterpret_cast<const double *>(d_features_in), iterations, sigma_c, sigma_n, sigma_a, sigma_d,
                        reinterpret_cast<double *>(d_out_linear), reinterpret_cast<unsigned char *>(d_out_rgb8), reinterpret_cast<double *>(d_out_stderr), st);
}

RTMI_EXPORT int rtmi_denoise(rtmi_ctx *c, int32_t nx, int32_t ny, const double *linear_in, const double *stderr_in, const double *features_in,
                             int32_t iterations, double sigma_c, double sigma_n, double sigma_a, double sigma_d,
                             double *out_linear, uint8_t *out_rgb8, double *out_stderr) {
    int rc = check_denoise_args(nx, ny, linear_in, iterations, sigma_c, sigma_n, sigma_a, sigma_d);
    if (rc) return rc;
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)nx * (size_t)ny;
    HostIo io(c);
    double *d_lin, *d_se, *d_feat, *d_olin, *d_ose;
    unsigned char *d_oq;
    io.in(&d_lin, 3 * n, linear_in); io.in(&d_se, n, stderr_in); io.in(&d_feat, 8 * n, features_in);
    io.out(&d_olin, 3 * n, out_linear); io.out(&d_oq, 3 * n, out_rgb8); io.out(&d_ose, n, out_stderr);
    rc = io.stage();
    if (!rc) rc = denoise_impl(c, nx, ny, d_lin, d_se, d_feat, iterations, sigma_c, sigma_n, sigma_a, sigma_d, d_olin, d_oq, d_ose, c->stream);
    return rc ? rc : io.finish();
}

// ---- temporal accumulation (rtmi_reproject*) -----------------------------------------------------------------------------------------------------------
namespace {
// the argument checks of both entries, before the handle is looked at: they need no device
int check_reproject_args(int nx, int ny, int prev_cam_kind, const double *prev_cam, int cur_cam_kind, const double *cur_cam, const void *prev_lin,
                         const void *prev_w, const void *prev_se, const void *prev_feat, const void *cur_lin, const void *cur_se, const void *cur_feat,
                         double cur_weight, double max_history, double sigma_d, double sigma_n, double sigma_a, const void *out_lin, const void *out_q,
                         const void *out_w, const void *out_se, const void *out_cnt) {
    if (nx <= 0 || ny <= 0) return fail(RTMI_E_ARG, "nx, ny must be > 0 (got %d %d)", nx, ny);
    if ((long long)nx * ny > (1ll << 30)) return fail(RTMI_E_ARG, "frame too large");
    if (!prev_cam) return fail(RTMI_E_ARG, "prev_cam is NULL");
    if (!cur_cam) return fail(RTMI_E_ARG, "cur_cam is NULL");
    const struct { const void *p; const char *name; } need[5] = {{prev_lin, "prev_linear"}, {prev_w, "prev_weight"}, {prev_feat, "prev_features"},
                                                                 {cur_lin, "cur_linear"}, {cur_feat, "cur_features"}};
    for (const auto &a : need)
        if (!a.p) return fail(RTMI_E_ARG, "%s is NULL", a.name);
    if (!(cur_weight > 0.0 && cur_weight < __builtin_inf())) return fail(RTMI_E_ARG, "cur_weight must be finite and > 0 (got %g)", cur_weight);
    if (!(max_history > 0.0)) return fail(RTMI_E_ARG, "max_history must be > 0 and not NaN (got %g)", max_history);
    const double sg[3] = {sigma_d, sigma_n, sigma_a};
    for (int k = 0; k < 3; ++k)
        if (!(sg[k] >= 0.0)) return fail(RTMI_E_ARG, "sigma_%c must be >= 0 and not NaN (got %g)", "dna"[k], sg[k]);
    if (out_se && !(prev_se && cur_se)) return fail(RTMI_E_ARG, "out_stderr needs both prev_stderr and cur_stderr");
    const struct { const void *p; const char *name; } outs[5] = {{out_lin, "out_linear"}, {out_q, "out_rgb8"}, {out_w, "out_weight"},
                                                                 {out_se, "out_stderr"}, {out_cnt, "out_counters"}};
    const struct { const void *p; const char *name; } prevs[4] = {{prev_lin, "prev_linear"}, {prev_w, "prev_weight"}, {prev_se, "prev_stderr"},
                                                                  {prev_feat, "prev_features"}};
    for (const auto &o : outs)
        for (const auto &q : prevs)
            if (o.p && o.p == q.p) return fail(RTMI_E_ARG, "%s is %s: the history is gathered from neighbours and cannot be overwritten in place", o.name, q.name);
    for (int kind : {prev_cam_kind, cur_cam_kind})
        if (kind != RTMI_CAM_PINHOLE && kind != RTMI_CAM_THINLENS) return fail(RTMI_E_UNSUPPORTED, "camera kind %d unsupported on GPU path", kind);
    return RTMI_OK;
}

// the launch: every pointer a device pointer, the cameras host arrays
int reproject_impl(int nx, int ny, const double *prev_cam, const double *cur_cam, const double *prev_lin, const double *prev_w, const double *prev_se,
                   const double *prev_feat, const double *cur_lin, const double *cur_se, const double *cur_feat, double cur_weight, double max_history,
                   double sigma_d, double sigma_n, double sigma_a, double *out_lin, unsigned char *out_q, double *out_w, double *out_se, u64 *out_cnt,
                   hipStream_t st) {
    ReprojectParams rp;
    rp.nx = nx; rp.ny = ny;
    rp.use_d = sigma_d > 0.0; rp.use_n = sigma_n > 0.0; rp.use_a = sigma_a > 0.0;
    double pl[3];
    for (int k = 0; k < 3; ++k) {
        rp.co[k] = cur_cam[k]; rp.cl[k] = cur_cam[3 + k]; rp.ch[k] = cur_cam[6 + k]; rp.cv[k] = cur_cam[9 + k];
        rp.po[k] = prev_cam[k]; pl[k] = prev_cam[3 + k]; rp.ph[k] = prev_cam[6 + k]; rp.pv[k] = prev_cam[9 + k];
        rp.a[k] = pl[k] - rp.po[k];
    }
    rp.n[0] = rp.ph[1] * rp.pv[2] - rp.ph[2] * rp.pv[1];
    rp.n[1] = rp.ph[2] * rp.pv[0] - rp.ph[0] * rp.pv[2];
    rp.n[2] = rp.ph[0] * rp.pv[1] - rp.ph[1] * rp.pv[0];
    rp.nn = (rp.n[0] * rp.n[0] + rp.n[1] * rp.n[1]) + rp.n[2] * rp.n[2];
    rp.A = (rp.a[0] * rp.n[0] + rp.a[1] * rp.n[1]) + rp.a[2] * rp.n[2];
    rp.cur_weight = cur_weight; rp.max_history = max_history;
    rp.sd2 = sigma_d * sigma_d; rp.sn2 = sigma_n * sigma_n; rp.sa2 = sigma_a * sigma_a;
    rp.prev_lin = prev_lin; rp.prev_w = prev_w; rp.prev_se = prev_se; rp.prev_feat = prev_feat;
    rp.cur_lin = cur_lin; rp.cur_se = cur_se; rp.cur_feat = cur_feat;
    rp.out_lin = out_lin; rp.out_q = out_q; rp.out_w = out_w; rp.out_se = out_se; rp.counters = out_cnt;
    if (out_cnt) HIP_TRY(hipMemsetAsync(out_cnt, 0, 2 * sizeof(u64), st));
    hipLaunchKernelGGL(reproject_kernel, dim3((unsigned)((nx + 63) / 64), (unsigned)((ny + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, st, rp);
    HIP_TRY(hipGetLastError());
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_reproject_device(rtmi_ctx *c, int32_t nx, int32_t ny, int32_t prev_cam_kind, const double *prev_cam, int32_t cur_cam_kind,
                                      const double *cur_cam, const void *d_prev_linear, const void *d_prev_weight, const void *d_prev_stderr,
                                      const void *d_prev_features, const void *d_cur_linear, const void *d_cur_stderr, const void *d_cur_features,
                                      double cur_weight, double max_history, double sigma_d, double sigma_n, double sigma_a, void *d_out_linear,
                                      void *d_out_rgb8, void *d_out_weight, void *d_out_stderr, void *d_out_counters, void *stream) {
    int rc = check_reproject_args(nx, ny, prev_cam_kind, prev_cam, cur_cam_kind, cur_cam, d_prev_linear, d_prev_weight, d_prev_stderr, d_prev_features,
                                  d_cur_linear, d_cur_stderr, d_cur_features, cur_weight, max_history, sigma_d, sigma_n, sigma_a, d_out_linear, d_out_rgb8,
                                  d_out_weight, d_out_stderr, d_out_counters);
    if (rc) return rc;
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    auto D = [](const void *p) { return reinterpret_cast<const double *>(p); };
    return reproject_impl(nx, ny, prev_cam, cur_cam, D(d_prev_linear), D(d_prev_weight), D(d_prev_stderr), D(d_prev_features), D(d_cur_linear),
                          D(d_cur_stderr), D(d_cur_features), cur_weight, max_history, sigma_d, sigma_n, sigma_a, reinterpret_cast<double *>(d_out_linear),
                          reinterpret_cast<unsigned char *>(d_out_rgb8), reinterpret_cast<double *>(d_out_weight), reinterpret_cast<double *>(d_out_stderr),
                          reinterpret_cast<u64 *>(d_out_counters), st);
}

RTMI_EXPORT int rtmi_reproject(rtmi_ctx *c, int32_t nx, int32_t ny, int32_t prev_cam_kind, const double *prev_cam, int32_t cur_cam_kind,
                               const double *cur_cam, const double *prev_linear, const double *prev_weight, const double *prev_stderr,
                               const double *prev_features, const double *cur_linear, const double *cur_stderr, const double *cur_features,
                               double cur_weight, double max_history, double sigma_d, double sigma_n, double sigma_a, double *out_linear,
                               uint8_t *out_rgb8, double *out_weight, double *out_stderr, uint64_t *out_counters) {
    int rc = check_reproject_args(nx, ny, prev_cam_kind, prev_cam, cur_cam_kind, cur_cam, prev_linear, prev_weight, prev_stderr, prev_features, cur_linear,
                                  cur_stderr, cur_features, cur_weight, max_history, sigma_d, sigma_n, sigma_a, out_linear, out_rgb8, out_weight, out_stderr,
                                  out_counters);
    if (rc) return rc;
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)nx * (size_t)ny;
    HostIo io(c);
    double *d_plin, *d_pw, *d_pse, *d_pft, *d_clin, *d_cse, *d_cft, *d_olin, *d_ow, *d_ose;
    unsigned char *d_oq;
    u64 *d_cnt;
    io.in(&d_plin, 3 * n, prev_linear); io.in(&d_pw, n, prev_weight); io.in(&d_pse, n, prev_stderr); io.in(&d_pft, 8 * n, prev_features);
    io.in(&d_clin, 3 * n, cur_linear); io.in(&d_cse, n, cur_stderr); io.in(&d_cft, 8 * n, cur_features);
    io.out(&d_olin, 3 * n, out_linear); io.out(&d_oq, 3 * n, out_rgb8); io.out(&d_ow, n, out_weight); io.out(&d_ose, n, out_stderr); io.out(&d_cnt, 2, out_counters);
    rc = io.stage();
    if (!rc) rc = reproject_impl(nx, ny, prev_cam, cur_cam, d_plin, d_pw, d_pse, d_pft, d_clin, d_cse, d_cft, cur_weight, max_history, sigma_d, sigma_n, sigma_a,
                                 d_olin, d_oq, d_ow, d_ose, d_cnt, c->stream);
    return rc ? rc : io.finish();
}

// ---- caller-supplied rays (rtmi_render_rays*) ---------------------------------------------------------------------------------------------------
namespace {
// rays_kernel's instantiations are chosen where the probe kernels' are (with_probe_kernel); the LDS-staged scans (scan_variant 0 / 1) need
// workgroup barriers and are answered with the scalar-cache scan, which finds the same hit (as the feature pass)
struct RaysPass {
    static constexpr bool wave_level = true;
    using Args = RaysParams; // the kernel's argument struct, and the RaysParams in it
    static RaysParams &rays(Args &a) { return a; }
    static constexpr int n_counters = 2;
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return rays_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT, MSEQ>; }
};
// rtmi_render_lit*, estimator 0: the same kernel building the frame's camera rays (SRC_CAMERA)
struct LitRaysPass : RaysPass {
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return rays_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT, MSEQ, SRC_CAMERA>; }
};
struct LitTilesRaysPass : RaysPass { // rtmi_render_lit_tiles*, estimator 0: the camera rays of a list of tiles (SRC_CAMERA_TILES)
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return rays_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT, MSEQ, SRC_CAMERA_TILES>; }
};
// The frame of a call whose rays the kernel builds (null for the calls that read theirs): what RaysParams holds of it.  out_camera is the call's.
// d_tiles (rtmi_render_lit_tiles*): the family's kernels are the SRC_CAMERA_TILES ones, the call's groups are the 64 pixel slots of each of its
// n_tiles entries in THE TILE ORDER, and the fold writes the listed pixels of the whole-frame state, mean, se and d_rgb8 (may be null).
struct RaysFrame { int nx, ny, fixed_rays; double *out_camera; const int *d_tiles = nullptr; int n_tiles = 0; unsigned char *d_rgb8 = nullptr; };

constexpr long long kRaysMax = (1ll << 31) - 64; // rays per call: 32-bit work items, and a claim past the end must not wrap the queue head

// The launches, all on `st`, every pointer a device pointer: passes of whole groups, each one launch of the family's kernel followed by its fold.  With
// d_out_rays the call is one pass into it; without, a pass holds as many groups as option "workspace_bytes" allows (at least one) in c->rays_ws.
// Family: RaysPass, or NeePass with upload_lights(args, st) queueing its table ahead of the passes.  c->counters: the family's counters when the
// caller passes no buffer, then the work-queue head.
struct NoLights { int operator()(RaysParams &, hipStream_t) const { return RTMI_OK; } };
template <typename R, typename Family, typename Lights>
int render_rays_impl(rtmi_scene *s, int n_groups, int group, int g_first, const double *d_rays, const u64 *d_keys, u64 seed, unsigned ctr0, int depth,
                     double *d_state, double *d_mean, double *d_se, double *d_out_rays, u64 *d_cnt, hipStream_t st, Lights upload_lights,
                     const RaysFrame *frame = nullptr) { // frame: the family's kernels are the SRC_CAMERA ones, d_rays and d_keys are null
    rtmi_ctx *c = s->ctx;
    int rc = c->counters.ensure(8 * sizeof(u64));
    if (rc) return rc;
    if (!d_cnt) d_cnt = reinterpret_cast<u64 *>(c->counters.p);
    const int *d_tiles = frame ? frame->d_tiles : nullptr;
    const int unit = d_tiles ? 64 : 1; // groups a pass is made of: a listed tile's 64 pixel slots stay together
    int per_pass = n_groups;
    if (!d_out_rays) {
        const int64_t group_bytes = (int64_t)group * 3 * (int64_t)sizeof(double);
        per_pass = (int)std::max<int64_t>(unit, std::min<int64_t>(n_groups, c->workspace_bytes / group_bytes / unit * unit));
        rc = c->rays_ws.ensure((size_t)per_pass * (size_t)group_bytes);
        if (rc) return rc;
    }
    typename Family::Args args;
    rc = upload_lights(args, st);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d_cnt, 0, Family::n_counters * sizeof(u64), st));
    RaysParams &rp = Family::rays(args);
    rp.seed = seed; rp.ctr0 = ctr0; rp.depth = depth;
    rp.group = (unsigned)group; rp.g_first = (unsigned)g_first;
    rp.queue = reinterpret_cast<unsigned *>(reinterpret_cast<u64 *>(c->counters.p) + Family::n_counters);
    rp.counters = d_cnt;
    rp.nx = frame ? frame->nx : 0; rp.ny = frame ? frame->ny : 0; rp.fixed_rays = frame ? frame->fixed_rays : 0; rp.out_camera = nullptr;
    rp.tiles = nullptr; rp.tiles_x = d_tiles ? tiles_x_of(rp.nx) : 0; rp.n_frame_tiles = d_tiles ? rp.tiles_x * tiles_x_of(rp.ny) : 0;
    const u64 n_rays = (u64)n_groups * (u64)group;
    with_probe_kernel<Family, R>(s, [&](auto kern, size_t lds, int, int) {
        for (int g0 = 0; g0 < n_groups && !rc; g0 += per_pass) {
            const int ng = std::min(per_pass, n_groups - g0);
            const size_t row0 = (size_t)g0 * (size_t)group;
            rp.rays = d_rays ? d_rays + row0 * 7 : nullptr;
            rp.keys = d_keys ? d_keys + row0 : nullptr;
            if (frame && frame->out_camera) rp.out_camera = frame->out_camera + row0 * 8;
            rp.samples = d_out_rays ? d_out_rays + row0 * 3 : reinterpret_cast<double *>(c->rays_ws.p);
            rp.row0 = (unsigned)row0;
            if (d_tiles) rp.tiles = d_tiles + g0 / 64;
            rc = queue_launch(c, st, reinterpret_cast<const void *>(kern), lds, rp.queue, (long long)ng * group,
                              [&](dim3 grid, unsigned items, unsigned qblock) {
                                  rp.total_items = items; rp.qblock = qblock;
                                  hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, st, s->d_dev, args);
                              },
                              [&] {
                                  const dim3 fold_grid((unsigned)((ng + kBlock - 1) / kBlock));
                                  if (d_tiles) {
                                      hipLaunchKernelGGL((lit_tiles_fold_kernel<R>), fold_grid, dim3(kBlock), 0, st, rp.samples, rp.tiles, ng / 64, group,
                                                         d_state ? g_first : 0, rp.tiles_x, rp.n_frame_tiles, rp.nx, rp.ny, d_state, d_mean, d_se, frame->d_rgb8);
                                      hipLaunchKernelGGL(lit_tiles_count_kernel, dim3(1), dim3(kCompactBlock), 0, st, rp.tiles, ng / 64, group, rp.tiles_x,
                                                         rp.n_frame_tiles, rp.nx, rp.ny, d_cnt);
                                  } else
                                      hipLaunchKernelGGL((rays_fold_kernel<R>), fold_grid, dim3(kBlock), 0, st, rp.samples, g0, ng, group,
                                                         d_state ? g_first : 0, d_state, d_mean, d_se, d_cnt, n_rays);
                              });
        }
    });
    return rc;
}

// What both forms of rtmi_render_rays* and rtmi_render_rays_nee* do first: the argument checks in the header's order (with T the light-sampling
// call's behind the plain call's: check_nee_args, beside its table below), a host form's state, then the scene's device is current.  *work
// false: nothing to trace, the entry returns RTMI_OK at once.
struct NeeLightTable;
int check_nee_args(rtmi_scene *s, int n_groups, int n_lights, const int32_t *light_prims, NeeLightTable &T, bool *work, int light_choice = 0, int vol = -1);
int rays_begin(rtmi_scene *s, int precision, int n_groups, int group, int g_first, int depth, const void *rays, const void *mean, const void *se,
               const double *host_state, bool *work, NeeLightTable *T = nullptr, int n_lights = 0, const int32_t *light_prims = nullptr,
               int light_choice = 0, bool generated = false, // generated: the kernel builds the rays (rtmi_render_lit*), `rays` is not looked at
               int vol = -1) {                               // vol >= 0: a call of the volume rule, vol its estimator argument
    *work = false;
    if (n_groups < 0 || group <= 0 || g_first < 0 || depth < 0)
        return fail(RTMI_E_ARG, "n_groups, g_first, depth must be >= 0 and group > 0 (got %d %d %d %d)", n_groups, g_first, depth, group);
    if ((long long)n_groups * group > kRaysMax) return fail(RTMI_E_ARG, "n_groups * group = %lld rays exceed 2^31 - 64", (long long)n_groups * group);
    if ((long long)g_first + group > INT32_MAX) return fail(RTMI_E_ARG, "g_first + group = %d + %d overflows int32", g_first, group);
    if (n_groups > 0 && !rays && !generated) return fail(RTMI_E_ARG, "rays is NULL");
    if (n_groups > 0 && (!mean || !se)) return fail(RTMI_E_ARG, "out_mean / out_stderr is NULL");
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    if (precision != RTMI_F64 && precision != RTMI_F32) return fail(RTMI_E_ARG, "precision must be RTMI_F64 or RTMI_F32");
    if (precision == RTMI_F32 && s->dev.has_ext) return fail(RTMI_E_UNSUPPORTED, "rectangles / triangles / instances / procedural textures are traced by the FP64 kernels only");
    if (s->uses_perlin && !s->have_perlin) return fail(RTMI_E_STATE, "the scene holds a Perlin texture: call rtmi_scene_set_perlin first");
    if (s->max_image >= s->dev.n_images) return fail(RTMI_E_STATE, "the scene holds an ImageMap with index %d: call rtmi_scene_set_images first", s->max_image);
    *work = n_groups > 0;
    int rc = T ? check_nee_args(s, n_groups, n_lights, light_prims, *T, work, light_choice, vol) : RTMI_OK;
    if (rc || !*work) return rc;
    rc = check_state_counts(host_state, (size_t)n_groups, RTMI_RAYS_REC, 9, g_first, "group", "rays, g_first");
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->ctx->device));
    return RTMI_OK;
}

int rays_run(rtmi_scene *s, int precision, int n_groups, int group, int g_first, const double *d_rays, const u64 *d_keys, u64 seed, unsigned ctr0, int depth,
             double *d_state, double *d_mean, double *d_se, double *d_out_rays, u64 *d_cnt, hipStream_t st) {
    return with_real(precision, [&](auto r) {
        return render_rays_impl<decltype(r), RaysPass>(s, n_groups, group, g_first, d_rays, d_keys, seed, ctr0, depth, d_state, d_mean, d_se, d_out_rays, d_cnt, st,
                                                       NoLights{});
    });
}
} // namespace

RTMI_EXPORT int rtmi_render_rays_device(rtmi_scene *s, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first, const void *d_rays,
                                        const void *d_keys, uint64_t seed, uint32_t ctr0, int32_t depth, void *d_state, void *d_out_mean,
                                        void *d_out_stderr, void *d_out_rays, void *d_out_counters, void *stream) {
    bool work = false;
    const int rc = rays_begin(s, precision, n_groups, group, g_first, depth, d_rays, d_out_mean, d_out_stderr, nullptr, &work);
    if (rc || !work) return rc;
    return rays_run(s, precision, n_groups, group, g_first, as<const double>(d_rays), as<const u64>(d_keys), seed, ctr0, depth, as<double>(d_state),
                    as<double>(d_out_mean), as<double>(d_out_stderr), as<double>(d_out_rays), as<u64>(d_out_counters), stream_of(s->ctx, stream));
}

RTMI_EXPORT int rtmi_render_rays(rtmi_scene *s, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first, const double *rays,
                                 const uint64_t *keys, uint64_t seed, uint32_t ctr0, int32_t depth, double *state, double *out_mean, double *out_stderr,
                                 double *out_rays, uint64_t *out_counters) {
    bool work = false;
    const int rc = rays_begin(s, precision, n_groups, group, g_first, depth, rays, out_mean, out_stderr, state, &work);
    if (rc || !work) return rc;
    const size_t n = (size_t)n_groups * (size_t)group, ng = (size_t)n_groups;
    HostIo io(s->ctx);
    double *d_rays, *d_state, *d_mean, *d_se, *d_out;
    u64 *d_keys, *d_cnt;
    io.in(&d_rays, 7 * n, rays); io.in(&d_keys, n, keys);
    io.plane(&d_state, ng * RTMI_RAYS_REC, state != nullptr, g_first > 0 ? state : nullptr, state); // a first chunk (g_first = 0) reads no records
    io.out(&d_mean, 3 * ng, out_mean); io.out(&d_se, ng, out_stderr); io.work(&d_cnt, 2, out_counters); io.out(&d_out, 3 * n, out_rays);
    return host_run(io, [&](hipStream_t st) {
        return rays_run(s, precision, n_groups, group, g_first, d_rays, d_keys, seed, ctr0, depth, d_state, d_mean, d_se, d_out, d_cnt, st);
    });
}

// ---- closest-hit and any-hit queries (rtmi_query_hits*, rtmi_query_occluded*) --------------------------------------------------------------------
namespace {
// query_kernel's instantiations are chosen where the probe kernels' are (with_probe_kernel), the LDS-staged scans answered with the scalar-cache scan as
// for rays_kernel.  COUNT (option "count_traversal") exists for the FP64 sphere tree only: every other family runs the kernel it always runs.
template <bool ANY, bool COUNT, int SRC = SRC_MEMORY> struct QueryPass {
    static constexpr bool wave_level = true;
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() {
        constexpr int W = V < SCAN_SGPR ? (int)SCAN_SGPR : V;
        return query_kernel<R, W, EXT, MSEQ, ANY, COUNT && W == SCAN_BVH && !EXT && std::is_same<R, double>::value, SRC>;
    }
};

// the argument checks of the four entries, in the header's order; out: the array a call cannot do without (null when it has none)
int check_query_args(rtmi_scene *s, int precision, long long n, bool dims_ok, const void *rays, bool out_ok) {
    if (!dims_ok) return fail(RTMI_E_ARG, "n, n_groups must be >= 0 and group > 0");
    if (n > kRaysMax) return fail(RTMI_E_ARG, "%lld rays exceed 2^31 - 64", n);
    if (n > 0 && !rays) return fail(RTMI_E_ARG, "rays is NULL");
    if (n > 0 && !out_ok) return fail(RTMI_E_ARG, "out_hits is NULL");
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    if (precision != RTMI_F64 && precision != RTMI_F32) return fail(RTMI_E_ARG, "precision must be RTMI_F64 or RTMI_F32");
    if (precision == RTMI_F32 && s->dev.has_ext) return fail(RTMI_E_UNSUPPORTED, "rectangles / triangles / instances are FP64 only");
    return RTMI_OK;
}

// The launch, on `st`, every pointer a device pointer: counters (and group counts) zeroed, then one query_kernel over the n rays.  gen: the src_* fields
// and out_rays of a generated source (SRC != SRC_MEMORY, which reads no d_rays).  fold: what reduces the kernel's output, inside its timing interval.
template <typename R, bool ANY, int SRC = SRC_MEMORY, typename Fold = NoFold>
int query_impl(rtmi_scene *s, int n, int n_groups, int group, const double *d_rays, const double *d_range, double t_min, double t_max, const u64 *d_keys,
               unsigned ctr0, double *d_hits, unsigned char *d_occ, int *d_count, u64 *d_cnt, hipStream_t st, const QueryParams *gen = nullptr,
               bool keep_counters = false, Fold fold = Fold{}) { // keep_counters: a later pass of one call adds to what its earlier passes counted
    rtmi_ctx *c = s->ctx;
    int rc = c->counters.ensure(8 * sizeof(u64)); // [0..1] the counters when the caller passes no buffer, [2] the work-queue head, [3..4] traversal counters
    if (rc) return rc;
    if (!d_cnt) d_cnt = reinterpret_cast<u64 *>(c->counters.p);
    if (!keep_counters) HIP_TRY(hipMemsetAsync(d_cnt, 0, 2 * sizeof(u64), st));
    if (ANY && d_count) HIP_TRY(hipMemsetAsync(d_count, 0, (size_t)n_groups * sizeof(int), st));
    const bool count = c->count_traversal != 0;
    if (count) {
        HIP_TRY(hipMemsetAsync(reinterpret_cast<u64 *>(c->counters.p) + 3, 0, 2 * sizeof(u64), st));
        c->last_stream = st;
    }
    QueryParams qp = gen ? *gen : QueryParams{};
    qp.rays = d_rays; qp.t_range = d_range; qp.keys = d_keys; qp.tmin = t_min; qp.tmax = t_max; qp.ctr0 = ctr0;
    qp.group = (unsigned)std::max(1, group);
    qp.queue = reinterpret_cast<unsigned *>(reinterpret_cast<u64 *>(c->counters.p) + 2);
    qp.hits = d_hits; qp.occluded = d_occ; qp.count = d_count; qp.counters = d_cnt;
    qp.trav = reinterpret_cast<u64 *>(c->counters.p) + 3;
    auto run = [&](auto kern, size_t lds, int, int) {
        rc = queue_launch(c, st, reinterpret_cast<const void *>(kern), lds, qp.queue, n,
                          [&](dim3 grid, unsigned items, unsigned qblock) {
                              qp.total_items = items; qp.qblock = qblock;
                              hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, st, s->d_dev, qp);
                          },
                          fold);
    };
    // a tree over a handful of mixed-kind primitives costs more than scanning them (choose_trace_kernel): the same shortcut, the same knobs
    const LaunchKnobs knobs = read_launch_knobs();
    const bool flat = s->dev.has_ext && !count && s->dev.n_all < (knobs.flat_below ? std::atoi(knobs.flat_below) : c->flat_below);
    if (count) with_probe_kernel<QueryPass<ANY, true, SRC>, R>(s, run);
    else with_probe_kernel<QueryPass<ANY, false, SRC>, R>(s, run, flat);
    return rc;
}

// what both forms of the two calls do first: the checks, then (with rays to trace) the scene's device is current
int query_begin(rtmi_scene *s, int precision, long long n, bool dims_ok, const void *rays, bool out_ok) {
    const int rc = check_query_args(s, precision, n, dims_ok, rays, out_ok);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(s->ctx->device));
    return RTMI_OK;
}
int query_hits_run(rtmi_scene *s, int precision, int n, const double *d_rays, const double *d_range, double t_min, double t_max, const u64 *d_keys,
                   unsigned ctr0, double *d_hits, u64 *d_cnt, hipStream_t st) {
    return with_real(precision, [&](auto r) {
        return query_impl<decltype(r), false>(s, n, 0, 1, d_rays, d_range, t_min, t_max, d_keys, ctr0, d_hits, nullptr, nullptr, d_cnt, st);
    });
}
int query_occluded_run(rtmi_scene *s, int precision, int n_groups, int group, const double *d_rays, const double *d_range, double t_min, double t_max,
                       const u64 *d_keys, unsigned ctr0, unsigned char *d_occ, int *d_count, u64 *d_cnt, hipStream_t st) {
    return with_real(precision, [&](auto r) {
        return query_impl<decltype(r), true>(s, n_groups * group, n_groups, group, d_rays, d_range, t_min, t_max, d_keys, ctr0, nullptr, d_occ, d_count, d_cnt, st);
    });
}
} // namespace

RTMI_EXPORT int rtmi_query_hits_device(rtmi_scene *s, int32_t precision, int32_t n, const void *d_rays, const void *d_t_range, double t_min, double t_max,
                                       const void *d_keys, uint32_t ctr0, void *d_out_hits, void *d_out_counters, void *stream) {
    const int rc = query_begin(s, precision, n, n >= 0, d_rays, d_out_hits != nullptr);
    if (rc || n == 0) return rc;
    return query_hits_run(s, precision, n, as<const double>(d_rays), as<const double>(d_t_range), t_min, t_max, as<const u64>(d_keys), ctr0,
                          as<double>(d_out_hits), as<u64>(d_out_counters), stream_of(s->ctx, stream));
}

RTMI_EXPORT int rtmi_query_hits(rtmi_scene *s, int32_t precision, int32_t n, const double *rays, const double *t_range, double t_min, double t_max,
                                const uint64_t *keys, uint32_t ctr0, double *out_hits, uint64_t *out_counters) {
    const int rc = query_begin(s, precision, n, n >= 0, rays, out_hits != nullptr);
    if (rc || n == 0) return rc;
    HostIo io(s->ctx);
    double *d_rays, *d_range, *d_hits;
    u64 *d_keys, *d_cnt;
    io.in(&d_rays, (size_t)n * 7, rays); io.in(&d_range, (size_t)n * 2, t_range); io.in(&d_keys, (size_t)n, keys);
    io.out(&d_hits, (size_t)n * RTMI_HIT_REC, out_hits); io.work(&d_cnt, 2, out_counters);
    return host_run(io, [&](hipStream_t st) { return query_hits_run(s, precision, n, d_rays, d_range, t_min, t_max, d_keys, ctr0, d_hits, d_cnt, st); });
}

RTMI_EXPORT int rtmi_query_occluded_device(rtmi_scene *s, int32_t precision, int32_t n_groups, int32_t group, const void *d_rays, const void *d_t_range,
                                           double t_min, double t_max, const void *d_keys, uint32_t ctr0, void *d_out_occluded, void *d_out_count,
                                           void *d_out_counters, void *stream) {
    const int rc = query_begin(s, precision, (long long)n_groups * group, n_groups >= 0 && group > 0, d_rays, true);
    if (rc || n_groups == 0) return rc;
    return query_occluded_run(s, precision, n_groups, group, as<const double>(d_rays), as<const double>(d_t_range), t_min, t_max, as<const u64>(d_keys), ctr0,
                              as<unsigned char>(d_out_occluded), as<int>(d_out_count), as<u64>(d_out_counters), stream_of(s->ctx, stream));
}

RTMI_EXPORT int rtmi_query_occluded(rtmi_scene *s, int32_t precision, int32_t n_groups, int32_t group, const double *rays, const double *t_range,
                                    double t_min, double t_max, const uint64_t *keys, uint32_t ctr0, uint8_t *out_occluded, int32_t *out_count,
                                    uint64_t *out_counters) {
    const int rc = query_begin(s, precision, (long long)n_groups * group, n_groups >= 0 && group > 0, rays, true);
    if (rc || n_groups == 0) return rc;
    const size_t n = (size_t)n_groups * (size_t)group;
    HostIo io(s->ctx);
    double *d_rays, *d_range;
    u64 *d_keys, *d_cnt;
    unsigned char *d_occ;
    int *d_count;
    io.in(&d_rays, n * 7, rays); io.in(&d_range, n * 2, t_range); io.in(&d_keys, n, keys);
    io.out(&d_occ, n, out_occluded); io.out(&d_count, (size_t)n_groups, out_count); io.work(&d_cnt, 2, out_counters);
    return host_run(io, [&](hipStream_t st) {
        return query_occluded_run(s, precision, n_groups, group, d_rays, d_range, t_min, t_max, d_keys, ctr0, d_occ, d_count, d_cnt, st);
    });
}

// ---- occlusion rays generated on the device (rtmi_occlusion_hemisphere*, rtmi_occlusion_targets*, rtmi_ambient_occlusion*) -------------------------
// query_kernel with a generated source: the points are rtmi_query_hits' records already in HBM, a ray is a few operations on its point's record, and no
// ray ever crosses the bus or lies in HBM unless the caller asks for it (out_rays).
namespace {
// visibility = 1 - occluded / n_dirs, and 1 where the primary ray missed
__global__ void __launch_bounds__(kBlock) ao_resolve_kernel(const double *__restrict__ hits, const int *__restrict__ count, int n, int n_dirs, double *__restrict__ vis) {
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= n) return;
    vis[p] = hits[(size_t)p * RTMI_HIT_REC] != 0.0 ? 1.0 - (double)count[p] / (double)n_dirs : 1.0;
}

// what both forms of the point entries do first: the argument checks, in the header's order, then (with points) the scene's device is current;
// per_point = n_dirs / n_targets
int occlusion_begin(rtmi_scene *s, int precision, int n_points, int per_point, int first, const void *hits, bool targets_ok) {
    if (n_points < 0 || per_point <= 0 || first < 0)
        return fail(RTMI_E_ARG, "n_points, first must be >= 0 and n_dirs / n_targets > 0 (got %d %d %d)", n_points, first, per_point);
    const long long n = (long long)n_points * per_point;
    if (n > kRaysMax) return fail(RTMI_E_ARG, "%lld rays exceed 2^31 - 64", n);
    if (n > 0 && !hits) return fail(RTMI_E_ARG, "hits is NULL");
    if (n > 0 && !targets_ok) return fail(RTMI_E_ARG, "targets is NULL");
    return query_begin(s, precision, n, true, hits, true); // the handle, the precision, RTMI_F32 on a mixed-kind scene
}

template <int SRC>
int occlusion_impl(rtmi_scene *s, int precision, int n_points, int per_point, const QueryParams &gen, double t_min, double t_max, unsigned char *d_occ,
                   int *d_count, u64 *d_cnt, hipStream_t st) {
    return with_real(precision, [&](auto r) {
        return query_impl<decltype(r), true, SRC>(s, n_points * per_point, n_points, per_point, nullptr, nullptr, t_min, t_max, nullptr, 0u, nullptr, d_occ,
                                                  d_count, d_cnt, st, &gen);
    });
}

QueryParams point_source(const double *d_hits, const double *d_view, const double *d_targets, int first, u64 seed, double time, double *d_out_rays) {
    QueryParams g{};
    g.src_hits = d_hits; g.src_view = d_view; g.src_targets = d_targets; g.src_first = (unsigned)first; g.src_seed = seed; g.src_time = time;
    g.out_rays = d_out_rays;
    return g;
}

int ao_begin(rtmi_scene *s, int precision, int nx, int ny, int n_dirs, int first, double radius, const void *vis) {
    if (nx < 0 || ny < 0 || n_dirs <= 0 || first < 0) return fail(RTMI_E_ARG, "nx, ny, first must be >= 0 and n_dirs > 0 (got %d %d %d %d)", nx, ny, first, n_dirs);
    if (!(radius > 0.0)) return fail(RTMI_E_ARG, "radius must be > 0 (got %g)", radius);
    const long long n = (long long)nx * ny;
    if (n > kRaysMax || n * n_dirs > kRaysMax) return fail(RTMI_E_ARG, "%lld pixels x %d rays exceed 2^31 - 64", n, n_dirs);
    if (n > 0 && !vis) return fail(RTMI_E_ARG, "out_visibility is NULL");
    return query_begin(s, precision, n, true, vis, true); // the handle, the precision, RTMI_F32 on a mixed-kind scene
}

// The whole pass on `st`: the first hits of the pixel-centre rays, n_dirs hemisphere rays per hit on the viewer's side (the pixel-centre ray is built
// again from the camera, not kept), the resolve.  d_hits / d_count null: in the context's workspace.
template <typename R>
int ao_impl(rtmi_scene *s, int nx, int ny, int n_dirs, int first, double radius, u64 seed, double *d_vis, int *d_count, double *d_hits, u64 *d_cnt,
            hipStream_t st) {
    rtmi_ctx *c = s->ctx;
    const size_t n = (size_t)nx * (size_t)ny, hit_bytes = n * RTMI_HIT_REC * sizeof(double);
    if (!d_hits || !d_count) {
        const int rc = c->occ_ws.ensure(hit_bytes + n * sizeof(int));
        if (rc) return rc;
        if (!d_hits) d_hits = reinterpret_cast<double *>(c->occ_ws.p);
        if (!d_count) d_count = reinterpret_cast<int *>(static_cast<char *>(c->occ_ws.p) + hit_bytes);
    }
    QueryParams g{};
    g.src_nx = (unsigned)nx; g.src_ny = (unsigned)ny;
    int rc = query_impl<R, false, SRC_PIXEL>(s, (int)n, 0, 1, nullptr, nullptr, 0.001, 3.4028234663852886e38, nullptr, 0u, d_hits, nullptr, nullptr, nullptr, st, &g);
    if (rc) return rc;
    g.src_hits = d_hits; g.src_first = (unsigned)first; g.src_seed = seed; g.src_view_camera = 1u;
    rc = query_impl<R, true, SRC_HEMISPHERE>(s, (int)(n * (size_t)n_dirs), (int)n, n_dirs, nullptr, nullptr, 0.001, radius, nullptr, 0u, nullptr, nullptr, d_count,
                                             d_cnt, st, &g);
    if (rc) return rc;
    hipLaunchKernelGGL(ao_resolve_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, d_hits, d_count, (int)n, n_dirs, d_vis);
    HIP_TRY(hipGetLastError());
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_occlusion_hemisphere_device(rtmi_scene *s, int32_t precision, int32_t n_points, const void *d_hits, const void *d_view, int32_t n_dirs,
                                                 int32_t first, uint64_t seed, double time, double t_min, double t_max, void *d_out_occluded,
                                                 void *d_out_count, void *d_out_rays, void *d_out_counters, void *stream) {
    const int rc = occlusion_begin(s, precision, n_points, n_dirs, first, d_hits, true);
    if (rc || n_points == 0) return rc;
    return occlusion_impl<SRC_HEMISPHERE>(s, precision, n_points, n_dirs,
                                          point_source(as<const double>(d_hits), as<const double>(d_view), nullptr, first, seed, time, as<double>(d_out_rays)),
                                          t_min, t_max, as<unsigned char>(d_out_occluded), as<int>(d_out_count), as<u64>(d_out_counters),
                                          stream_of(s->ctx, stream));
}

RTMI_EXPORT int rtmi_occlusion_hemisphere(rtmi_scene *s, int32_t precision, int32_t n_points, const double *hits, const double *view, int32_t n_dirs,
                                          int32_t first, uint64_t seed, double time, double t_min, double t_max, uint8_t *out_occluded, int32_t *out_count,
                                          double *out_rays, uint64_t *out_counters) {
    const int rc = occlusion_begin(s, precision, n_points, n_dirs, first, hits, true);
    if (rc || n_points == 0) return rc;
    const size_t np = (size_t)n_points, n = np * (size_t)n_dirs;
    HostIo io(s->ctx);
    double *d_hits, *d_view, *d_rays;
    u64 *d_cnt;
    unsigned char *d_occ;
    int *d_count;
    io.in(&d_hits, np * RTMI_HIT_REC, hits); io.in(&d_view, np * 7, view);
    io.out(&d_occ, n, out_occluded); io.out(&d_count, np, out_count); io.out(&d_rays, n * 7, out_rays); io.work(&d_cnt, 2, out_counters);
    return host_run(io, [&](hipStream_t st) {
        return occlusion_impl<SRC_HEMISPHERE>(s, precision, n_points, n_dirs, point_source(d_hits, d_view, nullptr, first, seed, time, d_rays), t_min, t_max,
                                              d_occ, d_count, d_cnt, st);
    });
}

RTMI_EXPORT int rtmi_occlusion_targets_device(rtmi_scene *s, int32_t precision, int32_t n_points, const void *d_hits, const void *d_view, int32_t n_targets,
                                              const void *d_targets, double time, double t_min, double t_max, void *d_out_occluded, void *d_out_count,
                                              void *d_out_rays, void *d_out_counters, void *stream) {
    const int rc = occlusion_begin(s, precision, n_points, n_targets, 0, d_hits, d_targets != nullptr);
    if (rc || n_points == 0) return rc;
    return occlusion_impl<SRC_TARGETS>(s, precision, n_points, n_targets,
                                       point_source(as<const double>(d_hits), as<const double>(d_view), as<const double>(d_targets), 0, 0ull, time,
                                                    as<double>(d_out_rays)),
                                       t_min, t_max, as<unsigned char>(d_out_occluded), as<int>(d_out_count), as<u64>(d_out_counters),
                                       stream_of(s->ctx, stream));
}

RTMI_EXPORT int rtmi_occlusion_targets(rtmi_scene *s, int32_t precision, int32_t n_points, const double *hits, const double *view, int32_t n_targets,
                                       const double *targets, double time, double t_min, double t_max, uint8_t *out_occluded, int32_t *out_count,
                                       double *out_rays, uint64_t *out_counters) {
    const int rc = occlusion_begin(s, precision, n_points, n_targets, 0, hits, targets != nullptr);
    if (rc || n_points == 0) return rc;
    const size_t np = (size_t)n_points, n = np * (size_t)n_targets;
    HostIo io(s->ctx);
    double *d_hits, *d_view, *d_targets, *d_rays;
    u64 *d_cnt;
    unsigned char *d_occ;
    int *d_count;
    io.in(&d_hits, np * RTMI_HIT_REC, hits); io.in(&d_view, np * 7, view); io.in(&d_targets, (size_t)n_targets * 3, targets);
    io.out(&d_occ, n, out_occluded); io.out(&d_count, np, out_count); io.out(&d_rays, n * 7, out_rays); io.work(&d_cnt, 2, out_counters);
    return host_run(io, [&](hipStream_t st) {
        return occlusion_impl<SRC_TARGETS>(s, precision, n_points, n_targets, point_source(d_hits, d_view, d_targets, 0, 0ull, time, d_rays), t_min, t_max,
                                           d_occ, d_count, d_cnt, st);
    });
}

namespace { // (behind the point entries: the kernels are instantiated in the order the calls were added in)
int ao_run(rtmi_scene *s, int precision, int nx, int ny, int n_dirs, int first, double radius, u64 seed, double *d_vis, int *d_count, double *d_hits,
           u64 *d_cnt, hipStream_t st) {
    return with_real(precision, [&](auto r) { return ao_impl<decltype(r)>(s, nx, ny, n_dirs, first, radius, seed, d_vis, d_count, d_hits, d_cnt, st); });
}
} // namespace

RTMI_EXPORT int rtmi_ambient_occlusion_device(rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t n_dirs, int32_t first, double radius,
                                              uint64_t seed, void *d_out_visibility, void *d_out_count, void *d_out_hits, void *d_out_counters, void *stream) {
    const int rc = ao_begin(s, precision, nx, ny, n_dirs, first, radius, d_out_visibility);
    if (rc || nx == 0 || ny == 0) return rc;
    return ao_run(s, precision, nx, ny, n_dirs, first, radius, seed, as<double>(d_out_visibility), as<int>(d_out_count), as<double>(d_out_hits),
                  as<u64>(d_out_counters), stream_of(s->ctx, stream));
}

RTMI_EXPORT int rtmi_ambient_occlusion(rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t n_dirs, int32_t first, double radius, uint64_t seed,
                                       double *out_visibility, int32_t *out_count, double *out_hits, uint64_t *out_counters) {
    const int rc = ao_begin(s, precision, nx, ny, n_dirs, first, radius, out_visibility);
    if (rc || nx == 0 || ny == 0) return rc;
    const size_t n = (size_t)nx * (size_t)ny;
    HostIo io(s->ctx);
    double *d_vis, *d_hits;
    u64 *d_cnt;
    int *d_count;
    io.out(&d_vis, n, out_visibility); io.out(&d_count, n, out_count); io.out(&d_hits, n * RTMI_HIT_REC, out_hits); io.work(&d_cnt, 2, out_counters);
    return host_run(io, [&](hipStream_t st) { return ao_run(s, precision, nx, ny, n_dirs, first, radius, seed, d_vis, d_count, d_hits, d_cnt, st); });
}

// ---- direct lighting from first hits (rtmi_scene_lights, rtmi_direct_irradiance*, rtmi_render_direct*) -------------------------------------------------
// query_kernel with SRC_LIGHT: a lane places a point on an area light, builds the shadow ray towards it and writes the item's contribution Le * w at once;
// after the any-hit search an occluded ray takes its contribution back (zeros), so no weight is alive across the search.  direct_fold_kernel sums a point's contributions in item order.  Which primitives are lights is read off
// the host-side tables the scene keeps (they follow every edit), and the table of the lights a call samples travels as kernel arguments.
namespace {
// the header's eligibility rule for primitive i of the flat arrays
bool light_eligible(const SceneArrays &a, int i) {
    const int kind = a.prim_kind[i];
    const double *g = a.prim_geom + (size_t)i * RTMI_PRIM_STRIDE;
    if (kind == RTMI_PRIM_SPHERE || kind == RTMI_PRIM_UVSPHERE) { if (!(g[3] > 0.0)) return false; }
    else if (kind == RTMI_PRIM_RECT_XY || kind == RTMI_PRIM_RECT_XZ || kind == RTMI_PRIM_RECT_YZ) { // both extents non-zero (a NaN is no extent)
        const double ea = g[2] - g[0], eb = g[3] - g[1];
        if (!(ea < 0.0 || ea > 0.0) || !(eb < 0.0 || eb > 0.0)) return false;
    }
    else return false; // (a RTMI_PRIM_BOUNDARY primitive has another kind value and ends here)
    if (a.prim_xform && a.prim_xform[2 * (size_t)i + 1] != 0) return false;
    const int m = a.prim_mat[i];
    if (m < 0 || m >= a.n_mats || a.mat_kind[m] != RTMI_MAT_DIFFUSE_LIGHT) return false;
    const int t = a.mat_tex[m];
    return t >= 0 && t < a.n_tex && a.tex_kind[t] == RTMI_TEX_CONSTANT;
}
int list_lights(const SceneArrays &a, int capacity, int32_t *out_prims, int32_t *out_count) {
    int n = 0;
    for (int i = 0; i < a.n_prims; ++i)
        if (light_eligible(a, i)) { if (n < capacity) out_prims[n] = i; ++n; }
    *out_count = n;
    return RTMI_OK;
}

struct LightTable { double rec[RTMI_DIRECT_MAX_LIGHTS * kLightRec]; int n, pad; };
// one wave stores the table where the query kernels queued behind it read it
__global__ void __launch_bounds__(64) set_lights_kernel(LightTable t, double *dst) {
    for (int i = (int)threadIdx.x; i < t.n * kLightRec; i += 64) dst[i] = t.rec[i];
}

// the lights of a call: the listed primitives, each eligible, or all eligible ones
int make_light_table(const rtmi_scene *s, int n_lights, const int32_t *light_prims, LightTable &T) {
    const SceneArrays a = kept_arrays(s);
    int32_t all[RTMI_DIRECT_MAX_LIGHTS];
    if (!light_prims) {
        int32_t count = 0;
        list_lights(a, RTMI_DIRECT_MAX_LIGHTS, all, &count);
        if (count > RTMI_DIRECT_MAX_LIGHTS) return fail(RTMI_E_ARG, "the scene holds %d eligible lights, a call samples at most %d: pass a list", count, RTMI_DIRECT_MAX_LIGHTS);
        n_lights = count; light_prims = all;
    }
    T.n = n_lights; T.pad = 0;
    for (int l = 0; l < n_lights; ++l) {
        const int i = light_prims[l];
        if (i < 0 || i >= a.n_prims || !light_eligible(a, i)) return fail(RTMI_E_ARG, "light_prims[%d] = %d is not an eligible light (rtmi_scene_lights)", l, i);
        const double *g = a.prim_geom + (size_t)i * RTMI_PRIM_STRIDE, *col = a.tex_param + (size_t)a.mat_tex[a.prim_mat[i]] * RTMI_TEX_STRIDE;
        double *r = T.rec + (size_t)l * kLightRec;
        const int kind = a.prim_kind[i];
        const bool sphere = kind == RTMI_PRIM_SPHERE || kind == RTMI_PRIM_UVSPHERE;
        r[0] = (double)kind;
        r[1] = g[0]; r[2] = g[1]; r[3] = g[2]; r[4] = g[3]; r[5] = sphere ? 0.0 : g[4];
        r[6] = sphere ? 0x1.921fb54442d18p+3 * (g[3] * g[3]) : std::fabs((g[2] - g[0]) * (g[3] - g[1]));
        r[7] = col[0]; r[8] = col[1]; r[9] = col[2];
    }
    return RTMI_OK;
}

// One lane per point of the pass (points [g0, g0 + n) of the call): the point's contributions in item order, starting FROM the first item of its first
// sample, then E = sum * (1 / samples).  state (may be null): {sum.rgb, samples}, read when first > 0 and written back; without one first is 0.
__global__ void __launch_bounds__(kBlock) direct_fold_kernel(const double *__restrict__ contrib, int g0, int n, int group, int first, int n_samples,
                                                             double *__restrict__ state, double *__restrict__ E) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n) return;
    const size_t g = (size_t)g0 + (size_t)gid;
    double acc[3] = {0.0, 0.0, 0.0};
    double *rec = state ? state + g * RTMI_DIRECT_REC : nullptr;
    if (rec && first > 0) { acc[0] = rec[0]; acc[1] = rec[1]; acc[2] = rec[2]; }
    const double *row = contrib + (size_t)gid * (size_t)group * 3;
    for (int i = 0; i < group; ++i, row += 3) {
        if (first == 0 && i == 0) { acc[0] = row[0]; acc[1] = row[1]; acc[2] = row[2]; }
        else { acc[0] = acc[0] + row[0]; acc[1] = acc[1] + row[1]; acc[2] = acc[2] + row[2]; }
    }
    const int samples = first + n_samples;
    if (rec) { rec[0] = acc[0]; rec[1] = acc[1]; rec[2] = acc[2]; rec[3] = (double)samples; }
    const double inv = 1.0 / (double)samples;
    E[g * 3] = acc[0] * inv; E[g * 3 + 1] = acc[1] * inv; E[g * 3 + 2] = acc[2] * inv;
}

// rtmi_render_direct's resolve: emitters show their emission, Lambertian surfaces (albedo * E) * INV_PI, everything else and a miss black
template <typename R, bool EXT>
__global__ void __launch_bounds__(kBlock) direct_resolve_kernel(ScenePtr scp, const double *__restrict__ hits, const double *__restrict__ E, int n, int n_mats,
                                                                double *__restrict__ out_linear, unsigned char *__restrict__ out_rgb8) {
    SceneRef sc = *scp;
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= n) return;
    const double *rec = hits + (size_t)p * RTMI_HIT_REC;
    double o[3] = {0.0, 0.0, 0.0};
    const double mf = rec[11];
    if (rec[0] != 0.0 && mf >= 0.0 && mf < (double)n_mats) {
        const int mat = (int)mf, mk = sc.mat_kind[mat];
        if (mk == RTMI_MAT_DIFFUSE_LIGHT || mk == RTMI_MAT_LAMBERTIAN) {
            R r, g, b;
            tex_sample<R, EXT>(sc, sc.mat_tex[mat], (R)rec[9], (R)rec[10], (R)rec[3], (R)rec[4], (R)rec[5], r, g, b);
            if (mk == RTMI_MAT_DIFFUSE_LIGHT) { o[0] = (double)r; o[1] = (double)g; o[2] = (double)b; }
            else {
                const double inv_pi = 0x1.45f306dc9c883p-2;
                o[0] = ((double)r * E[(size_t)p * 3]) * inv_pi; o[1] = ((double)g * E[(size_t)p * 3 + 1]) * inv_pi; o[2] = ((double)b * E[(size_t)p * 3 + 2]) * inv_pi;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (out_linear) out_linear[(size_t)p * 3 + c] = o[c];
        if (out_rgb8) out_rgb8[(size_t)p * 3 + c] = quantise8(o[c]);
    }
}

struct DirectView { const double *d_view; bool camera; int nx, ny; }; // the rays that found the points: an array, the pixel-centre rays built again, or none

// bytes of c->direct_ws: the light table, then whatever the caller lets the context hold, then one pass of contributions
constexpr size_t kLightTableBytes = sizeof(double) * RTMI_DIRECT_MAX_LIGHTS * kLightRec;

// The launches of the light passes on `st`, every pointer a device pointer: the table, then passes of whole points, each one query_kernel launch and its fold.
// d_contrib: the caller's [items][3] (one pass into it) or null: ws_contrib holds per_pass points.
template <typename R>
int direct_impl(rtmi_scene *s, int n_points, const double *d_hits, const DirectView &view, const LightTable &T, int n_samples, int first, u64 seed, double time,
                int lambert_only, double *d_state, double *d_E, double *d_contrib, unsigned char *d_occ, double *d_rays, u64 *d_cnt, double *ws_contrib,
                int per_pass, hipStream_t st) {
    rtmi_ctx *c = s->ctx;
    double *d_lights = reinterpret_cast<double *>(c->direct_ws.p);
    hipLaunchKernelGGL(set_lights_kernel, dim3(1), dim3(64), 0, st, T, d_lights);
    HIP_TRY(hipGetLastError());
    const int group = n_samples * T.n;
    QueryParams g{};
    g.src_lights = d_lights; g.src_n_lights = (unsigned)T.n; g.src_n_mats = (unsigned)s->n_mats; g.src_lambert = lambert_only ? 1u : 0u;
    g.src_first = (unsigned)first; g.src_seed = seed; g.src_time = time;
    g.src_view_camera = view.camera ? 1u : 0u; g.src_nx = (unsigned)view.nx; g.src_ny = (unsigned)view.ny;
    for (int g0 = 0; g0 < n_points; g0 += per_pass) {
        const int ng = std::min(per_pass, n_points - g0);
        const size_t row0 = (size_t)g0 * (size_t)group;
        g.src_g0 = (unsigned)g0;
        g.src_hits = d_hits + (size_t)g0 * RTMI_HIT_REC;
        g.src_view = view.d_view ? view.d_view + (size_t)g0 * 7 : nullptr;
        g.out_rays = d_rays ? d_rays + row0 * 7 : nullptr;
        g.contrib = d_contrib ? d_contrib + row0 * 3 : ws_contrib;
        const int rc = query_impl<R, true, SRC_LIGHT>(s, ng * group, ng, group, nullptr, nullptr, 0.001, 1.0 - 0.001, nullptr, 0u, nullptr,
                                                      d_occ ? d_occ + row0 : nullptr, nullptr, d_cnt, st, &g, g0 > 0, [&] {
            hipLaunchKernelGGL(direct_fold_kernel, dim3((unsigned)((ng + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, g.contrib, g0, ng, group,
                               d_state ? first : 0, n_samples, d_state, d_E);
        });
        if (rc) return rc;
    }
    return RTMI_OK;
}

// points of one pass and the bytes of its contributions in the workspace (none with the caller's out_contrib)
int direct_pass(const rtmi_ctx *c, int n_points, int group, bool own_contrib, size_t *bytes) {
    if (own_contrib) { *bytes = 0; return n_points; }
    const int64_t point_bytes = (int64_t)group * 3 * (int64_t)sizeof(double);
    const int per_pass = (int)std::max<int64_t>(1, std::min<int64_t>(n_points, c->workspace_bytes / point_bytes));
    *bytes = (size_t)per_pass * (size_t)point_bytes;
    return per_pass;
}

// Zero lights: nothing to sample.  Without a state the irradiance is zeros and nothing is launched.  With one, the fold runs over groups of no items: a
// point's sums carry over (zeros for a first chunk), its samples grow by n_samples and E = sum * (1 / samples), as if every sample had built no ray.
int direct_nothing(double *d_state, double *d_E, int n_points, int first, int n_samples, u64 *d_cnt, hipStream_t st) {
    if (d_cnt) HIP_TRY(hipMemsetAsync(d_cnt, 0, 2 * sizeof(u64), st));
    if (!d_state) { HIP_TRY(hipMemsetAsync(d_E, 0, (size_t)n_points * 3 * sizeof(double), st)); return RTMI_OK; }
    hipLaunchKernelGGL(direct_fold_kernel, dim3((unsigned)((n_points + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, static_cast<const double *>(nullptr), 0, n_points,
                       0, first, n_samples, d_state, d_E);
    HIP_TRY(hipGetLastError());
    return RTMI_OK;
}

int direct_irradiance_impl(rtmi_scene *s, int precision, int n_points, const double *d_hits, const double *d_view, const LightTable &T, int n_samples, int first,
                           u64 seed, double time, int lambert_only, double *d_state, double *d_E, double *d_contrib, unsigned char *d_occ, double *d_rays,
                           u64 *d_cnt, hipStream_t st) {
    rtmi_ctx *c = s->ctx;
    if (T.n == 0) return direct_nothing(d_state, d_E, n_points, first, n_samples, d_cnt, st);
    size_t pass_bytes = 0;
    const int per_pass = direct_pass(c, n_points, n_samples * T.n, d_contrib != nullptr, &pass_bytes);
    const int rc = c->direct_ws.ensure(kLightTableBytes + pass_bytes);
    if (rc) return rc;
    double *ws_contrib = reinterpret_cast<double *>(static_cast<char *>(c->direct_ws.p) + kLightTableBytes);
    const DirectView view{d_view, false, 0, 0};
    return with_real(precision, [&](auto r) {
        return direct_impl<decltype(r)>(s, n_points, d_hits, view, T, n_samples, first, seed, time, lambert_only, d_state, d_E, d_contrib, d_occ, d_rays, d_cnt,
                                        ws_contrib, per_pass, st);
    });
}

// The whole pass on `st`: the first hits of the pixel-centre rays, the light passes with those rays (built again from the camera) as the view, the resolve.
// d_hits null: the records live in the context's workspace, as the irradiance does.
template <typename R>
int render_direct_impl(rtmi_scene *s, int nx, int ny, const LightTable &T, int n_samples, int first, u64 seed, double *d_state, double *d_lin, unsigned char *d_q,
                       double *d_hits, u64 *d_cnt, hipStream_t st) {
    rtmi_ctx *c = s->ctx;
    const size_t n = (size_t)nx * (size_t)ny, hit_bytes = d_hits ? 0 : n * RTMI_HIT_REC * sizeof(double), e_bytes = n * 3 * sizeof(double);
    size_t pass_bytes = 0;
    const int per_pass = T.n ? direct_pass(c, (int)n, n_samples * T.n, false, &pass_bytes) : 0;
    int rc = c->direct_ws.ensure(kLightTableBytes + hit_bytes + e_bytes + pass_bytes);
    if (rc) return rc;
    char *ws = static_cast<char *>(c->direct_ws.p) + kLightTableBytes;
    if (!d_hits) d_hits = reinterpret_cast<double *>(ws);
    double *d_E = reinterpret_cast<double *>(ws + hit_bytes), *ws_contrib = reinterpret_cast<double *>(ws + hit_bytes + e_bytes);
    QueryParams g{};
    g.src_nx = (unsigned)nx; g.src_ny = (unsigned)ny;
    rc = query_impl<R, false, SRC_PIXEL>(s, (int)n, 0, 1, nullptr, nullptr, 0.001, 3.4028234663852886e38, nullptr, 0u, d_hits, nullptr, nullptr, nullptr, st, &g);
    if (rc) return rc;
    if (T.n == 0) rc = direct_nothing(d_state, d_E, (int)n, first, n_samples, d_cnt, st);
    else {
        const DirectView view{nullptr, true, nx, ny};
        rc = direct_impl<R>(s, (int)n, d_hits, view, T, n_samples, first, seed, 0.0, 1, d_state, d_E, nullptr, nullptr, nullptr, d_cnt, ws_contrib, per_pass, st);
    }
    if (rc) return rc;
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    if (s->dev.has_ext) hipLaunchKernelGGL((direct_resolve_kernel<double, true>), grid, dim3(kBlock), 0, st, s->d_dev, d_hits, d_E, (int)n, s->n_mats, d_lin, d_q);
    else hipLaunchKernelGGL((direct_resolve_kernel<R, false>), grid, dim3(kBlock), 0, st, s->d_dev, d_hits, d_E, (int)n, s->n_mats, d_lin, d_q);
    HIP_TRY(hipGetLastError());
    return RTMI_OK;
}
int render_direct_run(rtmi_scene *s, int precision, int nx, int ny, const LightTable &T, int n_samples, int first, u64 seed, double *d_state, double *d_lin,
                      unsigned char *d_q, double *d_hits, u64 *d_cnt, hipStream_t st) {
    return with_real(precision, [&](auto r) { return render_direct_impl<decltype(r)>(s, nx, ny, T, n_samples, first, seed, d_state, d_lin, d_q, d_hits, d_cnt, st); });
}

// What both forms of the two calls do first, in the header's order: the argument checks, the lights of the call in T, a host form's state, then the
// scene's device is current.  n_points = nx * ny for the whole pass (rtmi_render_direct*), whose resolve samples textures: what rtmi_render refuses
// for their tables, it refuses.  n_points = 0 passes: the entry returns RTMI_OK at once.
int direct_begin(rtmi_scene *s, int precision, long long n_points, bool dims_ok, int n_samples, int first, int n_lights, const int32_t *light_prims,
                 bool whole_pass, const void *hits, const void *out, const double *host_state, LightTable &T) {
    if (!dims_ok || n_samples <= 0 || first < 0) return fail(RTMI_E_ARG, "n_points (nx, ny), first must be >= 0 and n_samples > 0 (got %lld %d %d)", n_points, first, n_samples);
    if (light_prims && (n_lights < 0 || n_lights > RTMI_DIRECT_MAX_LIGHTS)) return fail(RTMI_E_ARG, "n_lights must be in [0, %d] (got %d)", RTMI_DIRECT_MAX_LIGHTS, n_lights);
    if (n_points > kRaysMax) return fail(RTMI_E_ARG, "%lld points exceed 2^31 - 64", n_points);
    if (n_points > 0 && !hits) return fail(RTMI_E_ARG, "hits is NULL");
    if (n_points > 0 && !out) return fail(RTMI_E_ARG, "out_irradiance / out_linear is NULL");
    int rc = check_query_args(s, precision, 0, true, nullptr, true); // the handle, the precision, RTMI_F32 on a mixed-kind scene
    if (rc || n_points == 0) return rc;
    if (whole_pass && s->uses_perlin && !s->have_perlin) return fail(RTMI_E_STATE, "the scene holds a Perlin texture: call rtmi_scene_set_perlin first");
    if (whole_pass && s->max_image >= s->dev.n_images) return fail(RTMI_E_STATE, "the scene holds an ImageMap with index %d: call rtmi_scene_set_images first", s->max_image);
    rc = make_light_table(s, n_lights, light_prims, T);
    if (rc) return rc;
    if ((long long)n_samples * T.n > kRaysMax || n_points * n_samples * T.n > kRaysMax)
        return fail(RTMI_E_ARG, "%lld points x %d samples x %d lights exceed 2^31 - 64 items", n_points, n_samples, T.n);
    rc = check_state_counts(host_state, (size_t)n_points, RTMI_DIRECT_REC, 3, first, whole_pass ? "pixel" : "point", "samples, first");
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->ctx->device));
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_scene_lights(rtmi_scene *s, int32_t capacity, int32_t *out_prims, int32_t *out_count) {
    if (capacity < 0 || !out_count || (capacity > 0 && !out_prims)) return fail(RTMI_E_ARG, "bad arguments");
    if (!scene_ok(s)) return fail(RTMI_E_STATE, "invalid scene handle");
    return list_lights(kept_arrays(s), capacity, out_prims, out_count);
}

RTMI_EXPORT int rtmi_test_scene_lights(int32_t n_prims, const int32_t *prim_kind, const double *prim_geom, const int32_t *prim_mat, int32_t n_mats,
                                       const int32_t *mat_kind, const int32_t *mat_tex, int32_t n_tex, const int32_t *tex_kind, const int32_t *prim_xform,
                                       int32_t capacity, int32_t *out_prims, int32_t *out_count) {
    if (capacity < 0 || !out_count || (capacity > 0 && !out_prims)) return fail(RTMI_E_ARG, "bad arguments");
    if (n_prims < 0 || n_mats < 0 || n_tex < 0 || (n_prims > 0 && (!prim_kind || !prim_geom || !prim_mat)) || (n_mats > 0 && (!mat_kind || !mat_tex)) || (n_tex > 0 && !tex_kind))
        return fail(RTMI_E_ARG, "a count is negative or an array is NULL");
    const SceneArrays a{n_prims, prim_kind, prim_geom, prim_mat, n_mats, mat_kind, mat_tex, nullptr, n_tex, tex_kind, nullptr, nullptr,
                        0, nullptr, nullptr, prim_xform, 0, nullptr, nullptr};
    return list_lights(a, capacity, out_prims, out_count);
}

RTMI_EXPORT int rtmi_direct_irradiance_device(rtmi_scene *s, int32_t precision, int32_t n_points, const void *d_hits, const void *d_view, int32_t n_lights,
                                              const int32_t *light_prims, int32_t n_samples, int32_t first, uint64_t seed, double time, int32_t lambert_only,
                                              void *d_state, void *d_out_irradiance, void *d_out_contrib, void *d_out_occluded, void *d_out_rays,
                                              void *d_out_counters, void *stream) {
    LightTable T;
    const int rc = direct_begin(s, precision, n_points, n_points >= 0, n_samples, first, n_lights, light_prims, false, d_hits, d_out_irradiance, nullptr, T);
    if (rc || n_points == 0) return rc;
    return direct_irradiance_impl(s, precision, n_points, as<const double>(d_hits), as<const double>(d_view), T, n_samples, first, seed, time, lambert_only,
                                  as<double>(d_state), as<double>(d_out_irradiance), as<double>(d_out_contrib), as<unsigned char>(d_out_occluded),
                                  as<double>(d_out_rays), as<u64>(d_out_counters), stream_of(s->ctx, stream));
}

RTMI_EXPORT int rtmi_direct_irradiance(rtmi_scene *s, int32_t precision, int32_t n_points, const double *hits, const double *view, int32_t n_lights,
                                       const int32_t *light_prims, int32_t n_samples, int32_t first, uint64_t seed, double time, int32_t lambert_only,
                                       double *state, double *out_irradiance, double *out_contrib, uint8_t *out_occluded, double *out_rays,
                                       uint64_t *out_counters) {
    LightTable T;
    const int rc = direct_begin(s, precision, n_points, n_points >= 0, n_samples, first, n_lights, light_prims, false, hits, out_irradiance, state, T);
    if (rc || n_points == 0) return rc;
    const size_t np = (size_t)n_points, n = np * (size_t)n_samples * (size_t)T.n;
    HostIo io(s->ctx);
    double *d_hits, *d_view, *d_state, *d_E, *d_contrib, *d_rays;
    unsigned char *d_occ;
    u64 *d_cnt;
    io.in(&d_hits, np * RTMI_HIT_REC, hits); io.in(&d_view, np * 7, view);
    io.plane(&d_state, np * RTMI_DIRECT_REC, state != nullptr, first > 0 ? state : nullptr, state); // a first chunk (first = 0) reads no records
    io.work(&d_E, np * 3, out_irradiance); io.out(&d_contrib, n * 3, n ? out_contrib : nullptr); io.out(&d_occ, n, n ? out_occluded : nullptr);
    io.out(&d_rays, n * 7, n ? out_rays : nullptr); io.work(&d_cnt, 2, out_counters);
    return host_run(io, [&](hipStream_t st) {
        return direct_irradiance_impl(s, precision, n_points, d_hits, d_view, T, n_samples, first, seed, time, lambert_only, d_state, d_E, d_contrib, d_occ, d_rays,
                                      d_cnt, st);
    });
}

RTMI_EXPORT int rtmi_render_direct_device(rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t n_samples, int32_t first, uint64_t seed, void *d_state,
                                          void *d_out_linear, void *d_out_rgb8, void *d_out_hits, void *d_out_counters, void *stream) {
    LightTable T;
    const int rc = direct_begin(s, precision, (long long)nx * ny, nx >= 0 && ny >= 0, n_samples, first, 0, nullptr, true, d_out_linear, d_out_linear, nullptr, T);
    if (rc || nx == 0 || ny == 0) return rc;
    return render_direct_run(s, precision, nx, ny, T, n_samples, first, seed, as<double>(d_state), as<double>(d_out_linear), as<unsigned char>(d_out_rgb8),
                             as<double>(d_out_hits), as<u64>(d_out_counters), stream_of(s->ctx, stream));
}

RTMI_EXPORT int rtmi_render_direct(rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t n_samples, int32_t first, uint64_t seed, double *state,
                                   double *out_linear, uint8_t *out_rgb8, double *out_hits, uint64_t *out_counters) {
    LightTable T;
    const int rc = direct_begin(s, precision, (long long)nx * ny, nx >= 0 && ny >= 0, n_samples, first, 0, nullptr, true, out_linear, out_linear, state, T);
    if (rc || nx == 0 || ny == 0) return rc;
    const size_t n = (size_t)nx * (size_t)ny;
    HostIo io(s->ctx);
    double *d_state, *d_lin, *d_hits;
    unsigned char *d_q;
    u64 *d_cnt;
    io.plane(&d_state, n * RTMI_DIRECT_REC, state != nullptr, first > 0 ? state : nullptr, state);
    io.work(&d_lin, n * 3, out_linear); io.out(&d_q, n * 3, out_rgb8); io.out(&d_hits, n * RTMI_HIT_REC, out_hits); io.work(&d_cnt, 2, out_counters);
    return host_run(io, [&](hipStream_t st) { return render_direct_run(s, precision, nx, ny, T, n_samples, first, seed, d_state, d_lin, d_q, d_hits, d_cnt, st); });
}

// ---- path tracing with next-event estimation (rtmi_render_rays_nee*, rtmi_probe_paths_nee) ---------------------------------------------------------
// rtmi_render_rays' passes and fold with rays_nee_kernel in rays_kernel's place.  The light table travels as the direct-lighting calls' does -- the
// arguments of a one-wave kernel, in stream order -- followed by the sampled lights' primitive indices, which the closing-emission rule compares with.
namespace {
struct NeePass {
    static constexpr bool wave_level = true;
    using Args = NeeParams;
    static RaysParams &rays(Args &a) { return a.rp; }
    static constexpr int n_counters = 4;
    // a media scene is refused before any launch, so the media-sequence operands of the chooser all name the one kernel
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return rays_nee_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT>; }
};
struct LitNeePass : NeePass { // rtmi_render_lit*, estimator 1: the frame's camera rays (SRC_CAMERA)
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return rays_nee_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT, false, SRC_CAMERA>; }
};
struct ProbePathsNee {
    static constexpr bool wave_level = true;
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return probe_paths_nee_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT>; }
};
// the MIS rule's instantiations of the two kernels (rtmi_render_rays_mis*, rtmi_probe_paths_mis)
struct MisPass : NeePass {
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return rays_nee_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT, true>; }
};
struct LitMisPass : NeePass { // rtmi_render_lit*, estimator 2
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return rays_nee_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT, true, SRC_CAMERA>; }
};
struct LitTilesNeePass : NeePass { // rtmi_render_lit_tiles*, estimators 1 and 2: the camera rays of a list of tiles (SRC_CAMERA_TILES)
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return rays_nee_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT, false, SRC_CAMERA_TILES>; }
};
struct LitTilesMisPass : NeePass {
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return rays_nee_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT, true, SRC_CAMERA_TILES>; }
};
struct ProbePathsMis {
    static constexpr bool wave_level = true;
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return probe_paths_nee_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT, true>; }
};
// THE VOLUME RULE's instantiations (rtmi_render_rays_vol*, rtmi_render_lit_vol*, rtmi_probe_paths_vol): VOL with the mixed-kind FP64 kernels, the only ones
// that trace a medium or an Isotropic scatter.  A world of spheres runs its sibling's kernel, which is then the same rule (the entries see to the probe's rows).
// A media scene outside RTMI_MEDIA_DESCENT is refused before any launch, so the media-sequence operands of the chooser all name the one kernel.
template <bool MIS, int SRC> struct VolPass : NeePass {
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return rays_nee_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT, MIS, SRC, EXT>; }
};
template <bool MIS> struct ProbePathsVol {
    static constexpr bool wave_level = true;
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return probe_paths_nee_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT, MIS, EXT>; }
};
// THE PROPOSAL RULE's instantiations (rtmi_render_rays_ris*, rtmi_render_lit_ris*, rtmi_probe_paths_ris): RIS on top of the MIS rule's kernels
template <int SRC> struct RisPass : NeePass {
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return rays_nee_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT, true, SRC, false, true>; }
};
struct ProbePathsRis {
    static constexpr bool wave_level = true;
    template <typename R, int V, bool EXT = false, int MSEQ = 0> static auto kernel() { return probe_paths_nee_kernel<R, (V < SCAN_SGPR ? (int)SCAN_SGPR : V), EXT, true, false, true>; }
};

struct NeeLightTable { LightTable t; int prim[RTMI_DIRECT_MAX_LIGHTS]; };
constexpr size_t kNeeLightBytes = kLightTableBytes + sizeof(int) * RTMI_DIRECT_MAX_LIGHTS;
__global__ void __launch_bounds__(64) set_nee_lights_kernel(NeeLightTable t, double *dst, int *dst_prim) {
    for (int i = (int)threadIdx.x; i < t.t.n * kLightRec; i += 64) dst[i] = t.t.rec[i];
    if ((int)threadIdx.x < t.t.n) dst_prim[threadIdx.x] = t.prim[threadIdx.x];
}

// the lights of a call and their primitives: the listed ones, each eligible, or all eligible ones
int make_nee_lights(const rtmi_scene *s, int n_lights, const int32_t *light_prims, NeeLightTable &T) {
    int32_t all[RTMI_DIRECT_MAX_LIGHTS];
    if (!light_prims) {
        int32_t count = 0;
        list_lights(kept_arrays(s), RTMI_DIRECT_MAX_LIGHTS, all, &count);
        if (count > RTMI_DIRECT_MAX_LIGHTS) return fail(RTMI_E_ARG, "the scene holds %d eligible lights, a call samples at most %d: pass a list", count, RTMI_DIRECT_MAX_LIGHTS);
        n_lights = count; light_prims = all;
    }
    const int rc = make_light_table(s, n_lights, light_prims, T.t);
    if (rc) return rc;
    for (int l = 0; l < RTMI_DIRECT_MAX_LIGHTS; ++l) T.prim[l] = l < n_lights ? light_prims[l] : -1;
    return RTMI_OK;
}

// the table on the device, queued on `st` ahead of the kernels that read it
int upload_nee_lights(rtmi_ctx *c, const NeeLightTable &T, NeeLights &L, hipStream_t st) {
    const int rc = c->nee_ws.ensure(kNeeLightBytes);
    if (rc) return rc;
    L.rec = reinterpret_cast<const double *>(c->nee_ws.p);
    L.prim = reinterpret_cast<const int *>(static_cast<const char *>(c->nee_ws.p) + kLightTableBytes);
    L.n = (unsigned)T.t.n;
    hipLaunchKernelGGL(set_nee_lights_kernel, dim3(1), dim3(64), 0, st, T, const_cast<double *>(L.rec), const_cast<int *>(L.prim));
    HIP_TRY(hipGetLastError());
    return RTMI_OK;
}

// The MIS calls' table: the NEE table, then the pick of the MIS rule's step 2 -- {W, -, then C_l, q_l per light} -- where the MIS instantiations read it
// (kMisRows).  It goes through a kernel of its own: what set_nee_lights_kernel stores is what it always stored.
constexpr int kMisWords = 2 + 2 * RTMI_DIRECT_MAX_LIGHTS;
struct MisLightTable { NeeLightTable t; double mis[kMisWords]; };
constexpr size_t kMisLightBytes = kNeeLightBytes + sizeof(double) * kMisWords;
static_assert(kNeeLightBytes == sizeof(double) * kMisRows, "the MIS rows start where the NEE table ends");
__global__ void __launch_bounds__(64) set_mis_lights_kernel(MisLightTable t, double *dst) {
    const int n = t.t.t.n;
    for (int i = (int)threadIdx.x; i < n * kLightRec; i += 64) dst[i] = t.t.t.rec[i];
    if ((int)threadIdx.x < n) reinterpret_cast<int *>(dst + RTMI_DIRECT_MAX_LIGHTS * kLightRec)[threadIdx.x] = t.t.prim[threadIdx.x];
    for (int i = (int)threadIdx.x; i < 2 + 2 * n; i += 64) dst[kMisRows + i] = t.mis[i];
}

// Step 2 of the MIS rule on the host: q_l = nl and W = 0 (the uniform pick) for light_choice 0, and for light_choice 1 whose W is not finite and > 0;
// else W, the running sums and q_l = W / omega_l.  A light by power with omega = 0 is never picked and is no sampled light for step 7: its primitive
// leaves the list the closing emitter is compared with.
void make_mis_rows(MisLightTable &T, int light_choice) {
    const int n = T.t.t.n;
    double *M = T.mis;
    M[0] = 0.0; M[1] = 0.0;
    for (int l = 0; l < RTMI_DIRECT_MAX_LIGHTS; ++l) { M[2 + 2 * l] = 0.0; M[3 + 2 * l] = (double)n; }
    if (light_choice != 1 || n == 0) return;
    double omega[RTMI_DIRECT_MAX_LIGHTS], cum[RTMI_DIRECT_MAX_LIGHTS];
    for (int l = 0; l < n; ++l) {
        const double *r = T.t.t.rec + (size_t)l * kLightRec;
        omega[l] = r[6] * ((r[7] + r[8]) + r[9]);
        cum[l] = l ? cum[l - 1] + omega[l] : omega[l];
    }
    const double W = cum[n - 1];
    if (!(std::isfinite(W) && W > 0.0)) return;
    M[0] = W;
    for (int l = 0; l < n; ++l) {
        M[2 + 2 * l] = cum[l]; M[3 + 2 * l] = W / omega[l];
        if (omega[l] == 0.0) T.t.prim[l] = -1;
    }
}

int upload_mis_lights(rtmi_ctx *c, const MisLightTable &T, NeeLights &L, hipStream_t st) {
    const int rc = c->nee_ws.ensure(kMisLightBytes);
    if (rc) return rc;
    L.rec = reinterpret_cast<const double *>(c->nee_ws.p);
    L.prim = reinterpret_cast<const int *>(static_cast<const char *>(c->nee_ws.p) + kLightTableBytes);
    L.n = (unsigned)T.t.t.n;
    hipLaunchKernelGGL(set_mis_lights_kernel, dim3(1), dim3(64), 0, st, T, const_cast<double *>(L.rec));
    HIP_TRY(hipGetLastError());
    return RTMI_OK;
}

// The RIS calls' table: the MIS table with q_l = 1.0 for every light (every light proposes: no pick), then lum_l where the RIS instantiations read it
// (kRisRows).  It goes through a kernel of its own: what the other two set-kernels store is what they always stored.
struct RisLightTable { MisLightTable m; double lum[RTMI_DIRECT_MAX_LIGHTS]; };
constexpr size_t kRisLightBytes = kMisLightBytes + sizeof(double) * RTMI_DIRECT_MAX_LIGHTS;
static_assert(kMisLightBytes == sizeof(double) * kRisRows, "the lum row starts where the MIS table ends");
static_assert(sizeof(RisLightTable) + 2 * sizeof(void *) <= 4096, "the table travels as a kernel's arguments");
__global__ void __launch_bounds__(64) set_ris_lights_kernel(RisLightTable t, double *dst) {
    const int n = t.m.t.t.n;
    for (int i = (int)threadIdx.x; i < n * kLightRec; i += 64) dst[i] = t.m.t.t.rec[i];
    if ((int)threadIdx.x < n) reinterpret_cast<int *>(dst + RTMI_DIRECT_MAX_LIGHTS * kLightRec)[threadIdx.x] = t.m.t.prim[threadIdx.x];
    for (int i = (int)threadIdx.x; i < 2 + 2 * n; i += 64) dst[kMisRows + i] = t.m.mis[i];
    if ((int)threadIdx.x < n) dst[kRisRows + threadIdx.x] = t.lum[threadIdx.x];
}

// Steps 2 and 7 of the proposal rule on the host: lum_l, q_l = 1.0, and a light whose lum is not > 0 -- it can never be chosen -- leaves the list the
// closing emitter is compared with.
void make_ris_rows(RisLightTable &T) {
    const int n = T.m.t.t.n;
    double *M = T.m.mis;
    M[0] = 0.0; M[1] = 0.0;
    for (int l = 0; l < RTMI_DIRECT_MAX_LIGHTS; ++l) {
        const double *r = T.m.t.t.rec + (size_t)l * kLightRec;
        M[2 + 2 * l] = 0.0; M[3 + 2 * l] = 1.0;
        T.lum[l] = l < n ? (r[7] + r[8]) + r[9] : 0.0;
        if (l < n && !(T.lum[l] > 0.0)) T.m.t.prim[l] = -1;
    }
}

int upload_ris_lights(rtmi_ctx *c, const RisLightTable &T, NeeLights &L, hipStream_t st) {
    const int rc = c->nee_ws.ensure(kRisLightBytes);
    if (rc) return rc;
    L.rec = reinterpret_cast<const double *>(c->nee_ws.p);
    L.prim = reinterpret_cast<const int *>(static_cast<const char *>(c->nee_ws.p) + kLightTableBytes);
    L.n = (unsigned)T.m.t.t.n;
    hipLaunchKernelGGL(set_ris_lights_kernel, dim3(1), dim3(64), 0, st, T, const_cast<double *>(L.rec));
    HIP_TRY(hipGetLastError());
    return RTMI_OK;
}

// what both entries check behind rtmi_render_rays' own checks, in the header's order; *work: is there anything to trace?
int check_nee_args(rtmi_scene *s, int n_groups, int n_lights, const int32_t *light_prims, NeeLightTable &T, bool *work, int light_choice, int vol) {
    *work = false;
    if (light_prims && (n_lights < 0 || n_lights > RTMI_DIRECT_MAX_LIGHTS)) return fail(RTMI_E_ARG, "n_lights must be in [0, %d] (got %d)", RTMI_DIRECT_MAX_LIGHTS, n_lights);
    if (vol >= 0 && vol != 1 && vol != 2) return fail(RTMI_E_ARG, "estimator must be 1 (the NEE rule) or 2 (the MIS rule) (got %d)", vol); // (the volume calls')
    if (light_choice != 0 && light_choice != 1) return fail(RTMI_E_ARG, "light_choice must be 0 (uniform) or 1 (by power) (got %d)", light_choice); // (the MIS calls')
    if (n_groups == 0) return RTMI_OK;
    if (vol >= 0) { // the volume rule takes the media of a RTMI_MEDIA_DESCENT world; the list forms need MSEQ kernels this family does not have
        if (s->dev.n_media > 0 && s->dev.media_seq != 0)
            return fail(RTMI_E_UNSUPPORTED, "the scene holds a ConstantMedium in a Hitlist (media mode %d): the volume rule covers RTMI_MEDIA_DESCENT only", s->dev.media_seq);
    } else
    if (s->dev.n_media > 0) return fail(RTMI_E_UNSUPPORTED, "the scene holds a ConstantMedium: shadow rays through media are not built");
    *work = true;
    return make_nee_lights(s, n_lights, light_prims, T);
}

// the passes with the light-sampling kernel; no light to sample: the call is rtmi_render_rays and its two shadow-ray counters are zeros
int nee_run(rtmi_scene *s, int precision, int n_groups, int group, int g_first, const double *d_rays, const u64 *d_keys, u64 seed, unsigned ctr0, int depth,
            const NeeLightTable &T, double *d_state, double *d_mean, double *d_se, double *d_out_rays, u64 *d_cnt, hipStream_t st,
            const MisLightTable *M = nullptr, // M (then T is M->t): the MIS rule's kernels and table
            const RaysFrame *frame = nullptr, // frame: the SRC_CAMERA twins of the three families (rtmi_render_lit*), or with a list their SRC_CAMERA_TILES twins
            bool vol = false,                 // vol: the volume rule's instantiations of the two light-sampling families
            const RisLightTable *Rs = nullptr) { // Rs (then T is Rs->m.t): the proposal rule's kernels and table
    return with_real(precision, [&](auto r) {
        using R = decltype(r);
        auto ris_lights = [&](NeeParams &np, hipStream_t q) { return upload_ris_lights(s->ctx, *Rs, np.lights, q); };
        auto mis_lights = [&](NeeParams &np, hipStream_t q) { return upload_mis_lights(s->ctx, *M, np.lights, q); };
        auto nee_lights = [&](NeeParams &np, hipStream_t q) { return upload_nee_lights(s->ctx, T, np.lights, q); };
        // the family's kernels by the source of the rays: the caller's array, the frame's camera rays, those of a list of tiles
        auto run = [&](auto camera, auto memory, auto tiles, auto lights) {
            auto go = [&](auto family) {
                return render_rays_impl<R, decltype(family)>(s, n_groups, group, g_first, d_rays, d_keys, seed, ctr0, depth, d_state, d_mean, d_se, d_out_rays, d_cnt,
                                                             st, lights, frame);
            };
            return frame && !frame->d_tiles ? go(camera) : !frame ? go(memory) : go(tiles);
        };
        if (Rs && T.t.n > 0) return run(RisPass<SRC_CAMERA>{}, RisPass<SRC_MEMORY>{}, RisPass<SRC_CAMERA_TILES>{}, ris_lights);
        if (vol && M && T.t.n > 0) return run(VolPass<true, SRC_CAMERA>{}, VolPass<true, SRC_MEMORY>{}, VolPass<true, SRC_CAMERA_TILES>{}, mis_lights);
        if (vol && T.t.n > 0) return run(VolPass<false, SRC_CAMERA>{}, VolPass<false, SRC_MEMORY>{}, VolPass<false, SRC_CAMERA_TILES>{}, nee_lights);
        if (M && T.t.n > 0) return run(LitMisPass{}, MisPass{}, LitTilesMisPass{}, mis_lights);
        if (T.t.n > 0) return run(LitNeePass{}, NeePass{}, LitTilesNeePass{}, nee_lights);
        if (d_cnt) HIP_TRY(hipMemsetAsync(d_cnt + 2, 0, 2 * sizeof(u64), st));
        return run(LitRaysPass{}, RaysPass{}, LitTilesRaysPass{}, NoLights{});
    });
}

// The three entries of both families.  mis: the MIS rule with light_choice; else the NEE rule (light_choice is 0).  vol >= 0: the volume rule's entries,
// vol their estimator argument (mis is then vol == 2).
int lit_rays_device(bool mis, rtmi_scene *s, int precision, int n_groups, int group, int g_first, const void *d_rays, const void *d_keys, u64 seed, unsigned ctr0,
                    int depth, int n_lights, const int32_t *light_prims, int light_choice, void *d_state, void *d_out_mean, void *d_out_stderr, void *d_out_rays,
                    void *d_out_counters, void *stream, int vol = -1, bool ris = false) {
    RisLightTable Rt;
    MisLightTable &M = Rt.m;
    NeeLightTable &T = M.t;
    bool work = false;
    const int rc = rays_begin(s, precision, n_groups, group, g_first, depth, d_rays, d_out_mean, d_out_stderr, nullptr, &work, &T, n_lights, light_prims, light_choice,
                              false, vol);
    if (rc || !work) return rc;
    if (mis) make_mis_rows(M, light_choice);
    if (ris) make_ris_rows(Rt);
    return nee_run(s, precision, n_groups, group, g_first, as<const double>(d_rays), as<const u64>(d_keys), seed, ctr0, depth, T, as<double>(d_state),
                   as<double>(d_out_mean), as<double>(d_out_stderr), as<double>(d_out_rays), as<u64>(d_out_counters), stream_of(s->ctx, stream), mis ? &M : nullptr,
                   nullptr, vol >= 0, ris ? &Rt : nullptr);
}

int lit_rays_host(bool mis, rtmi_scene *s, int precision, int n_groups, int group, int g_first, const double *rays, const uint64_t *keys, u64 seed, unsigned ctr0,
                  int depth, int n_lights, const int32_t *light_prims, int light_choice, double *state, double *out_mean, double *out_stderr, double *out_rays,
                  uint64_t *out_counters, int vol = -1, bool ris = false) {
    RisLightTable Rt;
    MisLightTable &M = Rt.m;
    NeeLightTable &T = M.t;
    bool work = false;
    const int rc = rays_begin(s, precision, n_groups, group, g_first, depth, rays, out_mean, out_stderr, state, &work, &T, n_lights, light_prims, light_choice, false,
                              vol);
    if (rc || !work) return rc;
    if (mis) make_mis_rows(M, light_choice);
    if (ris) make_ris_rows(Rt);
    const size_t n = (size_t)n_groups * (size_t)group, ng = (size_t)n_groups;
    HostIo io(s->ctx);
    double *d_rays, *d_state, *d_mean, *d_se, *d_out;
    u64 *d_keys, *d_cnt;
    io.in(&d_rays, 7 * n, rays); io.in(&d_keys, n, keys);
    io.plane(&d_state, ng * RTMI_RAYS_REC, state != nullptr, g_first > 0 ? state : nullptr, state); // a first chunk (g_first = 0) reads no records
    io.out(&d_mean, 3 * ng, out_mean); io.out(&d_se, ng, out_stderr); io.work(&d_cnt, 4, out_counters); io.out(&d_out, 3 * n, out_rays);
    return host_run(io, [&](hipStream_t st) {
        return nee_run(s, precision, n_groups, group, g_first, d_rays, d_keys, seed, ctr0, depth, T, d_state, d_mean, d_se, d_out, d_cnt, st, mis ? &M : nullptr,
                       nullptr, vol >= 0, ris ? &Rt : nullptr);
    });
}

// out_dropped (the NEE probe: int32 flags) or out_weight (the MIS probe: doubles), whichever the family writes per path.  vol >= 0: rtmi_probe_paths_vol,
// vol its estimator argument (mis is then vol == 2): RTMI_VOL_REC rows and out_weight under either rule.
int lit_probe(bool mis, rtmi_scene *s, int precision, int n, const double *rays, const uint64_t *keys, u64 ctr0, int depth, int n_lights, const int32_t *light_prims,
              int light_choice, double *out_rgb, uint64_t *out_nseg, int32_t *out_dropped, double *out_weight, double *log, int max_seg, int32_t *out_nlog,
              int vol = -1, bool ris = false) { // ris: rtmi_probe_paths_ris (mis is then true, light_choice 0): RTMI_RIS_REC rows
    int rc = probe_begin(s, precision, n);
    if (rc || n == 0) return rc;
    if (!rays || !keys || !out_rgb) return fail(RTMI_E_ARG, "NULL array");
    if (log && max_seg <= 0) return fail(RTMI_E_ARG, "log given but max_seg <= 0");
    if (precision == RTMI_F32 && s->dev.has_ext) return fail(RTMI_E_UNSUPPORTED, "rectangles / triangles / instances are FP64 only");
    RisLightTable Rt;
    MisLightTable &M = Rt.m;
    NeeLightTable &T = M.t;
    bool work = false;
    rc = check_nee_args(s, n, n_lights, light_prims, T, &work, light_choice, vol);
    if (rc) return rc;
    if (vol >= 0 && !s->dev.has_ext) { // a world of spheres: no medium, no Isotropic scatter -- the sibling's probe is the rule; its rows are widened here
        const int kSib = mis ? RTMI_MIS_REC : RTMI_NEE_REC;
        std::vector<double> rows(log ? (size_t)n * max_seg * kSib : 0);
        std::vector<int32_t> dropped(mis || !out_weight ? 0 : (size_t)n);
        rc = lit_probe(mis, s, precision, n, rays, keys, ctr0, depth, n_lights, light_prims, light_choice, out_rgb, out_nseg, dropped.empty() ? nullptr : dropped.data(),
                       mis ? out_weight : nullptr, log ? rows.data() : nullptr, max_seg, out_nlog);
        if (rc) return rc;
        for (size_t k = 0; k < dropped.size(); ++k) out_weight[k] = dropped[k] ? 0.0 : 1.0;
        for (size_t v = 0; log && v < (size_t)n * max_seg; ++v)
            for (int c = 0; c < RTMI_VOL_REC; ++c) log[v * RTMI_VOL_REC + c] = c < kSib ? rows[v * kSib + c] : 0.0;
        return RTMI_OK;
    }
    if (mis) make_mis_rows(M, light_choice);
    if (ris) make_ris_rows(Rt);
    rtmi_ctx *c = s->ctx;
    HostIo io(c);
    NeeProbeParams pp{};
    double *d_rays, *d_rgb, *d_log, *d_weight;
    u64 *d_keys, *d_nseg;
    int *d_dropped, *d_nlog;
    const size_t log_words = log ? (size_t)n * max_seg * (ris ? RTMI_RIS_REC : vol >= 0 ? RTMI_VOL_REC : mis ? RTMI_MIS_REC : RTMI_NEE_REC) : 0;
    io.in(&d_rays, (size_t)n * 7, rays); io.in(&d_keys, (size_t)n, keys); io.out(&d_rgb, (size_t)n * 3, out_rgb);
    io.out(&d_nseg, (size_t)n, out_nseg); io.out(&d_dropped, (size_t)n, out_dropped); io.out(&d_weight, (size_t)n, out_weight); io.out(&d_nlog, (size_t)n, out_nlog);
    io.out(&d_log, log_words, log);
    pp.n = n; pp.ctr0 = (unsigned)ctr0; pp.depth = depth; pp.max_seg = max_seg;
    return probe_run(io, n, [&](hipStream_t st, dim3 grid) {
        pp.rays = d_rays; pp.keys = d_keys; pp.out_rgb = d_rgb; pp.out_nseg = d_nseg; pp.out_nlog = d_nlog; pp.log = d_log;
        pp.out_end = mis || vol >= 0 ? static_cast<void *>(d_weight) : static_cast<void *>(d_dropped);
        if ((ris ? upload_ris_lights(c, Rt, pp.lights, st) : mis ? upload_mis_lights(c, M, pp.lights, st) : upload_nee_lights(c, T, pp.lights, st)) != RTMI_OK) return; // (probe_run reports a launch error)
        if (d_log && hipMemsetAsync(d_log, 0, log_words * sizeof(double), st) != hipSuccess) return;
        auto run = [&](auto kern, size_t lds, int, int) { hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, st, s->d_dev, pp); };
        with_real(precision, [&](auto r) {
            if (ris) with_probe_kernel<ProbePathsRis, decltype(r)>(s, run);
            else if (vol >= 0 && mis) with_probe_kernel<ProbePathsVol<true>, decltype(r)>(s, run);
            else if (vol >= 0) with_probe_kernel<ProbePathsVol<false>, decltype(r)>(s, run);
            else if (mis) with_probe_kernel<ProbePathsMis, decltype(r)>(s, run);
            else with_probe_kernel<ProbePathsNee, decltype(r)>(s, run);
        });
    });
}
} // namespace

RTMI_EXPORT int rtmi_render_rays_nee_device(rtmi_scene *s, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first, const void *d_rays,
                                            const void *d_keys, uint64_t seed, uint32_t ctr0, int32_t depth, int32_t n_lights, const int32_t *light_prims,
                                            void *d_state, void *d_out_mean, void *d_out_stderr, void *d_out_rays, void *d_out_counters, void *stream) {
    return lit_rays_device(false, s, precision, n_groups, group, g_first, d_rays, d_keys, seed, ctr0, depth, n_lights, light_prims, 0, d_state, d_out_mean,
                           d_out_stderr, d_out_rays, d_out_counters, stream);
}

RTMI_EXPORT int rtmi_render_rays_nee(rtmi_scene *s, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first, const double *rays,
                                     const uint64_t *keys, uint64_t seed, uint32_t ctr0, int32_t depth, int32_t n_lights, const int32_t *light_prims,
                                     double *state, double *out_mean, double *out_stderr, double *out_rays, uint64_t *out_counters) {
    return lit_rays_host(false, s, precision, n_groups, group, g_first, rays, keys, seed, ctr0, depth, n_lights, light_prims, 0, state, out_mean, out_stderr,
                         out_rays, out_counters);
}

RTMI_EXPORT int rtmi_probe_paths_nee(rtmi_scene *s, int32_t precision, int32_t n, const double *rays, const uint64_t *keys, uint64_t ctr0, int32_t depth,
                                     int32_t n_lights, const int32_t *light_prims, double *out_rgb, uint64_t *out_nseg, int32_t *out_dropped, double *log,
                                     int32_t max_seg, int32_t *out_nlog) {
    return lit_probe(false, s, precision, n, rays, keys, ctr0, depth, n_lights, light_prims, 0, out_rgb, out_nseg, out_dropped, nullptr, log, max_seg, out_nlog);
}

// ---- multiple importance sampling for the light-sampled paths (rtmi_render_rays_mis*, rtmi_probe_paths_mis): THE MIS RULE of rtmi.h ---------------------
RTMI_EXPORT int rtmi_render_rays_mis_device(rtmi_scene *s, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first, const void *d_rays,
                                            const void *d_keys, uint64_t seed, uint32_t ctr0, int32_t depth, int32_t n_lights, const int32_t *light_prims,
                                            int32_t light_choice, void *d_state, void *d_out_mean, void *d_out_stderr, void *d_out_rays, void *d_out_counters,
                                            void *stream) {
    return lit_rays_device(true, s, precision, n_groups, group, g_first, d_rays, d_keys, seed, ctr0, depth, n_lights, light_prims, light_choice, d_state,
                           d_out_mean, d_out_stderr, d_out_rays, d_out_counters, stream);
}

RTMI_EXPORT int rtmi_render_rays_mis(rtmi_scene *s, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first, const double *rays,
                                     const uint64_t *keys, uint64_t seed, uint32_t ctr0, int32_t depth, int32_t n_lights, const int32_t *light_prims,
                                     int32_t light_choice, double *state, double *out_mean, double *out_stderr, double *out_rays, uint64_t *out_counters) {
    return lit_rays_host(true, s, precision, n_groups, group, g_first, rays, keys, seed, ctr0, depth, n_lights, light_prims, light_choice, state, out_mean,
                         out_stderr, out_rays, out_counters);
}

RTMI_EXPORT int rtmi_probe_paths_mis(rtmi_scene *s, int32_t precision, int32_t n, const double *rays, const uint64_t *keys, uint64_t ctr0, int32_t depth,
                                     int32_t n_lights, const int32_t *light_prims, int32_t light_choice, double *out_rgb, uint64_t *out_nseg, double *out_weight,
                                     double *log, int32_t max_seg, int32_t *out_nlog) {
    return lit_probe(true, s, precision, n, rays, keys, ctr0, depth, n_lights, light_prims, light_choice, out_rgb, out_nseg, nullptr, out_weight, log, max_seg,
                     out_nlog);
}

// ---- light-sampled frames from the scene's camera (rtmi_render_lit*): THE FRAME RULE of rtmi.h -----------------------------------------------------------
// rtmi_render_rays* / _nee* / _mis* with n_groups = nx * ny, g_first = s_first, group = s_count and the SRC_CAMERA twins of their kernels: no ray is
// read, a refilled lane builds start_sample's.  Everything behind the checks is nee_run's.
namespace {
// what both forms check first, in the header's order; *M: estimators 1 and 2's light table (estimator 0: no light); *work false: nothing to do
// vol: rtmi_render_lit_vol* -- the light-sampling calls' checks run for every estimator, the volume rule's own (estimators 1 and 2 only) behind the list's length
// tl: rtmi_render_lit_tiles* -- the list as the caller gave it (a host form's is checked entry by entry, a device form's is the caller's contract; the
// kernels give an entry outside the frame no pixel); the volume rule is then tl->volume, and the rows of the call are the listed tiles' 64 * s_count each
struct LitTileArgs { int volume, n_tiles; const int32_t *host_tiles; const void *tiles; };
int lit_frame_begin(rtmi_scene *s, int precision, int nx, int ny, int s_first, int s_count, int depth, int estimator, int n_lights, const int32_t *light_prims,
                    int light_choice, const double *host_state, const void *out_linear, const void *out_stderr, MisLightTable &M, RaysFrame &F, bool *work,
                    bool vol = false, const LitTileArgs *tl = nullptr) {
    *work = false;
    if (nx <= 0 || ny <= 0 || s_count <= 0 || s_first < 0 || depth < 0)
        return fail(RTMI_E_ARG, "nx, ny, s_count must be > 0 and s_first, depth >= 0 (got %d %d %d %d %d)", nx, ny, s_count, s_first, depth);
    if (tl && ((long long)nx * ny > kRaysMax || (tl->n_tiles > 0 && (long long)tl->n_tiles * 64 > kRaysMax / s_count)))
        return fail(RTMI_E_ARG, "n_tiles * 64 * s_count = %d * 64 * %d rays (or nx * ny = %d * %d pixels) exceed 2^31 - 64", tl->n_tiles, s_count, nx, ny);
    if (!tl && ((long long)nx * ny > kRaysMax || (long long)nx * ny * s_count > kRaysMax))
        return fail(RTMI_E_ARG, "nx * ny * s_count = %d * %d * %d rays exceed 2^31 - 64", nx, ny, s_count);
    if ((long long)s_first + s_count > INT32_MAX) return fail(RTMI_E_ARG, "s_first + s_count = %d + %d overflows int32", s_first, s_count);
    if (!out_linear || !out_stderr) return fail(RTMI_E_ARG, "out_linear / out_stderr is NULL");
    if (estimator < 0 || estimator > 2) return fail(RTMI_E_ARG, "estimator must be 0 (plain), 1 (the NEE rule) or 2 (the MIS rule) (got %d)", estimator);
    const int tiles_x = tiles_x_of(nx), n_frame_tiles = tiles_x * tiles_x_of(ny);
    if (tl) {
        if (tl->volume != 0 && tl->volume != 1) return fail(RTMI_E_ARG, "volume must be 0 (rtmi_render_lit's rules) or 1 (rtmi_render_lit_vol's) (got %d)", tl->volume);
        if (tl->n_tiles < 0 || (tl->n_tiles > 0 && !tl->tiles)) return fail(RTMI_E_ARG, "n_tiles must be >= 0 and tiles not NULL (got %d)", tl->n_tiles);
        for (int k = 0; tl->host_tiles && k < tl->n_tiles; ++k) {
            const int t = tl->host_tiles[k];
            if (t < 0 || t >= n_frame_tiles) return fail(RTMI_E_ARG, "tiles[%d] = %d, the frame has %d tiles", k, t, n_frame_tiles);
            if (k && t <= tl->host_tiles[k - 1]) return fail(RTMI_E_ARG, "tiles[%d] = %d follows %d: the list must be strictly ascending", k, t, tl->host_tiles[k - 1]);
        }
    }
    M.t.t.n = 0;
    const int rc = rays_begin(s, precision, tl ? tl->n_tiles * 64 : nx * ny, s_count, s_first, depth, nullptr, out_linear, out_stderr, tl ? nullptr : host_state, work,
                              estimator || vol ? &M.t : nullptr, n_lights, light_prims, estimator == 2 ? light_choice : 0, true, vol ? estimator : -1);
    if (rc || !*work) return rc;
    for (int k = 0; tl && tl->host_tiles && host_state && s_first > 0 && k < tl->n_tiles; ++k) { // the listed pixels' records continue at s_first
        const int t = tl->host_tiles[k], x0 = (t % tiles_x) * RTMI_TILE, y0 = (t / tiles_x) * RTMI_TILE;
        for (int y = y0; y < std::min(y0 + RTMI_TILE, ny); ++y)
            for (int x = x0; x < std::min(x0 + RTMI_TILE, nx); ++x) {
                const double held = host_state[((size_t)y * (size_t)nx + (size_t)x) * RTMI_RAYS_REC + 9];
                if (held != (double)s_first) return fail(RTMI_E_STATE, "pixel (%d, %d) of tile %d holds %g samples, s_first is %d", x, y, t, held, s_first);
            }
    }
    if (estimator == 2) make_mis_rows(M, light_choice);
    F.nx = nx; F.ny = ny; F.fixed_rays = camera_fixed_rays(s->dev.cam_kind, s->dev.cam_fixed_origin, s->dev.cam);
    F.n_tiles = tl ? tl->n_tiles : 0;
    return RTMI_OK;
}

int lit_frame_run(rtmi_scene *s, int precision, int nx, int ny, int s_first, int s_count, int depth, u64 seed, int estimator, const MisLightTable &M,
                  const RaysFrame &F, double *d_state, double *d_lin, unsigned char *d_q, double *d_se, double *d_out_rays, u64 *d_cnt, hipStream_t st,
                  bool vol = false, const RisLightTable *Rs = nullptr) { // Rs (then M is Rs->m): the proposal rule
    const int rc = nee_run(s, precision, F.d_tiles ? F.n_tiles * 64 : nx * ny, s_count, s_first, nullptr, nullptr, seed, 0u, depth, M.t, d_state, d_lin, d_se,
                           d_out_rays, d_cnt, st, estimator == 2 ? &M : nullptr, &F, vol, Rs);
    if (rc || !d_q || F.d_tiles) return rc; // (a list: the tile fold has quantised the pixels it wrote, F.d_rgb8)
    const size_t n = (size_t)nx * (size_t)ny * 3;
    hipLaunchKernelGGL(lit_quantise_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, d_lin, n, d_q);
    HIP_TRY(hipGetLastError());
    return RTMI_OK;
}
} // namespace

namespace {
// both forms of rtmi_render_lit* and, with vol, of rtmi_render_lit_vol*; ris: rtmi_render_lit_ris* without a list (the MIS rule's checks, light_choice 0)
int lit_frame_device(bool vol, rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                     int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice, void *d_state, void *d_out_linear, void *d_out_rgb8,
                     void *d_out_stderr, void *d_out_rays, void *d_out_camera, void *d_out_counters, void *stream, bool ris = false) {
    RisLightTable Rt;
    MisLightTable &M = Rt.m;
    RaysFrame F;
    bool work = false;
    const int rc = lit_frame_begin(s, precision, nx, ny, s_first, s_count, depth, estimator, n_lights, light_prims, light_choice, nullptr, d_out_linear,
                                   d_out_stderr, M, F, &work, vol);
    if (rc || !work) return rc;
    if (ris) make_ris_rows(Rt);
    F.out_camera = as<double>(d_out_camera);
    return lit_frame_run(s, precision, nx, ny, s_first, s_count, depth, seed, estimator, M, F, as<double>(d_state), as<double>(d_out_linear),
                         as<unsigned char>(d_out_rgb8), as<double>(d_out_stderr), as<double>(d_out_rays), as<u64>(d_out_counters), stream_of(s->ctx, stream), vol,
                         ris ? &Rt : nullptr);
}

int lit_frame_host(bool vol, rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                   int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice, double *state, double *out_linear,
                   uint8_t *out_rgb8, double *out_stderr, double *out_rays, double *out_camera, uint64_t *out_counters, bool ris = false) {
    RisLightTable Rt;
    MisLightTable &M = Rt.m;
    RaysFrame F;
    bool work = false;
    const int rc = lit_frame_begin(s, precision, nx, ny, s_first, s_count, depth, estimator, n_lights, light_prims, light_choice, state, out_linear, out_stderr,
                                   M, F, &work, vol);
    if (rc || !work) return rc;
    if (ris) make_ris_rows(Rt);
    const size_t ng = (size_t)nx * (size_t)ny, n = ng * (size_t)s_count;
    HostIo io(s->ctx);
    double *d_state, *d_lin, *d_se, *d_out, *d_cam;
    unsigned char *d_q;
    u64 *d_cnt;
    io.plane(&d_state, ng * RTMI_RAYS_REC, state != nullptr, s_first > 0 ? state : nullptr, state); // a first chunk (s_first = 0) reads no records
    io.out(&d_lin, 3 * ng, out_linear); io.out(&d_se, ng, out_stderr); io.out(&d_q, 3 * ng, out_rgb8); io.work(&d_cnt, 4, out_counters);
    io.out(&d_out, 3 * n, out_rays); io.out(&d_cam, 8 * n, out_camera);
    return host_run(io, [&](hipStream_t st) {
        F.out_camera = d_cam;
        return lit_frame_run(s, precision, nx, ny, s_first, s_count, depth, seed, estimator, M, F, d_state, d_lin, d_q, d_se, d_out, d_cnt, st, vol,
                             ris ? &Rt : nullptr);
    });
}
} // namespace

RTMI_EXPORT int rtmi_render_lit_device(rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                                       int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice, void *d_state,
                                       void *d_out_linear, void *d_out_rgb8, void *d_out_stderr, void *d_out_rays, void *d_out_camera, void *d_out_counters,
                                       void *stream) {
    return lit_frame_device(false, s, precision, nx, ny, s_first, s_count, depth, seed, estimator, n_lights, light_prims, light_choice, d_state, d_out_linear,
                            d_out_rgb8, d_out_stderr, d_out_rays, d_out_camera, d_out_counters, stream);
}

RTMI_EXPORT int rtmi_render_lit(rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                                int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice, double *state, double *out_linear,
                                uint8_t *out_rgb8, double *out_stderr, double *out_rays, double *out_camera, uint64_t *out_counters) {
    return lit_frame_host(false, s, precision, nx, ny, s_first, s_count, depth, seed, estimator, n_lights, light_prims, light_choice, state, out_linear, out_rgb8,
                          out_stderr, out_rays, out_camera, out_counters);
}

// ---- light-sampled paths and frames through participating media (rtmi_render_rays_vol*, rtmi_probe_paths_vol, rtmi_render_lit_vol*): THE VOLUME RULE ------
// The siblings' entries with the VOL instantiations of their kernels.  estimator 1: the NEE rule (light_choice is not looked at), 2: the MIS rule.
RTMI_EXPORT int rtmi_render_rays_vol_device(rtmi_scene *s, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first, const void *d_rays,
                                            const void *d_keys, uint64_t seed, uint32_t ctr0, int32_t depth, int32_t estimator, int32_t n_lights,
                                            const int32_t *light_prims, int32_t light_choice, void *d_state, void *d_out_mean, void *d_out_stderr, void *d_out_rays,
                                            void *d_out_counters, void *stream) {
    return lit_rays_device(estimator == 2, s, precision, n_groups, group, g_first, d_rays, d_keys, seed, ctr0, depth, n_lights, light_prims,
                           estimator == 2 ? light_choice : 0, d_state, d_out_mean, d_out_stderr, d_out_rays, d_out_counters, stream, estimator < 0 ? 0 : estimator);
}

RTMI_EXPORT int rtmi_render_rays_vol(rtmi_scene *s, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first, const double *rays,
                                     const uint64_t *keys, uint64_t seed, uint32_t ctr0, int32_t depth, int32_t estimator, int32_t n_lights,
                                     const int32_t *light_prims, int32_t light_choice, double *state, double *out_mean, double *out_stderr, double *out_rays,
                                     uint64_t *out_counters) {
    return lit_rays_host(estimator == 2, s, precision, n_groups, group, g_first, rays, keys, seed, ctr0, depth, n_lights, light_prims,
                         estimator == 2 ? light_choice : 0, state, out_mean, out_stderr, out_rays, out_counters, estimator < 0 ? 0 : estimator);
}

RTMI_EXPORT int rtmi_probe_paths_vol(rtmi_scene *s, int32_t precision, int32_t n, const double *rays, const uint64_t *keys, uint64_t ctr0, int32_t depth,
                                     int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice, double *out_rgb, uint64_t *out_nseg,
                                     double *out_weight, double *log, int32_t max_seg, int32_t *out_nlog) {
    return lit_probe(estimator == 2, s, precision, n, rays, keys, ctr0, depth, n_lights, light_prims, estimator == 2 ? light_choice : 0, out_rgb, out_nseg, nullptr,
                     out_weight, log, max_seg, out_nlog, estimator < 0 ? 0 : estimator);
}

RTMI_EXPORT int rtmi_render_lit_vol_device(rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth,
                                           uint64_t seed, int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice, void *d_state,
                                           void *d_out_linear, void *d_out_rgb8, void *d_out_stderr, void *d_out_rays, void *d_out_camera, void *d_out_counters,
                                           void *stream) {
    return lit_frame_device(true, s, precision, nx, ny, s_first, s_count, depth, seed, estimator, n_lights, light_prims, light_choice, d_state, d_out_linear,
                            d_out_rgb8, d_out_stderr, d_out_rays, d_out_camera, d_out_counters, stream);
}

RTMI_EXPORT int rtmi_render_lit_vol(rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                                    int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice, double *state, double *out_linear,
                                    uint8_t *out_rgb8, double *out_stderr, double *out_rays, double *out_camera, uint64_t *out_counters) {
    return lit_frame_host(true, s, precision, nx, ny, s_first, s_count, depth, seed, estimator, n_lights, light_prims, light_choice, state, out_linear, out_rgb8,
                          out_stderr, out_rays, out_camera, out_counters);
}

// ---- light-sampled frames over a caller's list of 8x8 tiles (rtmi_render_lit_tiles*): THE TILE ORDER of rtmi.h --------------------------------------------
// rtmi_render_lit* / rtmi_render_lit_vol* with the SRC_CAMERA_TILES twins of their kernels and lit_tiles_fold_kernel behind each pass: the rows of the call
// are the listed tiles' pixels, the frame planes and the state stay the whole frame's and only the listed pixels' elements are touched.
namespace {
// both forms of rtmi_render_lit_tiles*; ris: rtmi_render_lit_ris* with a list (the MIS rule's checks, light_choice 0, volume 0)
int lit_tiles_device(rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth,
                     uint64_t seed, int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice, int32_t volume,
                     int32_t n_tiles, const void *d_tiles, void *d_state, void *d_out_linear, void *d_out_rgb8, void *d_out_stderr,
                     void *d_out_rays, void *d_out_camera, void *d_out_counters, void *stream, bool ris = false) {
    RisLightTable Rt;
    MisLightTable &M = Rt.m;
    RaysFrame F;
    bool work = false;
    const LitTileArgs tl{volume, n_tiles, nullptr, d_tiles};
    const int rc = lit_frame_begin(s, precision, nx, ny, s_first, s_count, depth, estimator, n_lights, light_prims, light_choice, nullptr, d_out_linear,
                                   d_out_stderr, M, F, &work, volume == 1, &tl);
    if (rc || !work) return rc;
    if (ris) make_ris_rows(Rt);
    F.out_camera = as<double>(d_out_camera); F.d_tiles = as<const int>(d_tiles); F.d_rgb8 = as<unsigned char>(d_out_rgb8);
    return lit_frame_run(s, precision, nx, ny, s_first, s_count, depth, seed, estimator, M, F, as<double>(d_state), as<double>(d_out_linear),
                         as<unsigned char>(d_out_rgb8), as<double>(d_out_stderr), as<double>(d_out_rays), as<u64>(d_out_counters), stream_of(s->ctx, stream),
                         volume == 1, ris ? &Rt : nullptr);
}

// The host form stages the whole planes both ways: the elements outside the list come back with the bits they went up with.
int lit_tiles_host(rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                   int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice, int32_t volume, int32_t n_tiles,
                   const int32_t *tiles, double *state, double *out_linear, uint8_t *out_rgb8, double *out_stderr, double *out_rays,
                   double *out_camera, uint64_t *out_counters, bool ris = false) {
    RisLightTable Rt;
    MisLightTable &M = Rt.m;
    RaysFrame F;
    bool work = false;
    const LitTileArgs tl{volume, n_tiles, tiles, tiles};
    const int rc = lit_frame_begin(s, precision, nx, ny, s_first, s_count, depth, estimator, n_lights, light_prims, light_choice, state, out_linear, out_stderr,
                                   M, F, &work, volume == 1, &tl);
    if (rc || !work) return rc;
    if (ris) make_ris_rows(Rt);
    const size_t ng = (size_t)nx * (size_t)ny, n = (size_t)n_tiles * 64 * (size_t)s_count;
    HostIo io(s->ctx);
    double *d_state, *d_lin, *d_se, *d_out, *d_cam;
    unsigned char *d_q;
    u64 *d_cnt;
    int *d_tiles;
    io.in(&d_tiles, (size_t)n_tiles, tiles);
    io.plane(&d_state, ng * RTMI_RAYS_REC, state != nullptr, state, state);
    io.plane(&d_lin, 3 * ng, true, out_linear, out_linear); io.plane(&d_se, ng, true, out_stderr, out_stderr);
    io.plane(&d_q, 3 * ng, out_rgb8 != nullptr, out_rgb8, out_rgb8); io.work(&d_cnt, 4, out_counters);
    io.out(&d_out, 3 * n, out_rays); io.out(&d_cam, 8 * n, out_camera);
    return host_run(io, [&](hipStream_t st) {
        F.out_camera = d_cam; F.d_tiles = d_tiles; F.d_rgb8 = d_q;
        return lit_frame_run(s, precision, nx, ny, s_first, s_count, depth, seed, estimator, M, F, d_state, d_lin, d_q, d_se, d_out, d_cnt, st, volume == 1,
                             ris ? &Rt : nullptr);
    });
}
} // namespace

RTMI_EXPORT int rtmi_render_lit_tiles_device(rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth,
                                             uint64_t seed, int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice, int32_t volume,
                                             int32_t n_tiles, const void *d_tiles, void *d_state, void *d_out_linear, void *d_out_rgb8, void *d_out_stderr,
                                             void *d_out_rays, void *d_out_camera, void *d_out_counters, void *stream) {
    return lit_tiles_device(s, precision, nx, ny, s_first, s_count, depth, seed, estimator, n_lights, light_prims, light_choice, volume, n_tiles, d_tiles, d_state,
                            d_out_linear, d_out_rgb8, d_out_stderr, d_out_rays, d_out_camera, d_out_counters, stream);
}

RTMI_EXPORT int rtmi_render_lit_tiles(rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                                      int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice, int32_t volume, int32_t n_tiles,
                                      const int32_t *tiles, double *state, double *out_linear, uint8_t *out_rgb8, double *out_stderr, double *out_rays,
                                      double *out_camera, uint64_t *out_counters) {
    return lit_tiles_host(s, precision, nx, ny, s_first, s_count, depth, seed, estimator, n_lights, light_prims, light_choice, volume, n_tiles, tiles, state,
                          out_linear, out_rgb8, out_stderr, out_rays, out_camera, out_counters);
}

// ---- light-sampled paths whose every lamp proposes a point (rtmi_render_rays_ris*, rtmi_probe_paths_ris, rtmi_render_lit_ris*): THE PROPOSAL RULE -------
// The MIS siblings' entries with the RIS instantiations of their kernels: the MIS rule's checks with light_choice 0, then the table with q = 1 and lum.
// The frame call without a list runs the SRC_CAMERA kernels (rtmi_render_lit's rows and layouts), with a list the SRC_CAMERA_TILES ones.
RTMI_EXPORT int rtmi_render_rays_ris_device(rtmi_scene *s, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first, const void *d_rays,
                                            const void *d_keys, uint64_t seed, uint32_t ctr0, int32_t depth, int32_t n_lights, const int32_t *light_prims,
                                            void *d_state, void *d_out_mean, void *d_out_stderr, void *d_out_rays, void *d_out_counters, void *stream) {
    return lit_rays_device(true, s, precision, n_groups, group, g_first, d_rays, d_keys, seed, ctr0, depth, n_lights, light_prims, 0, d_state, d_out_mean,
                           d_out_stderr, d_out_rays, d_out_counters, stream, -1, true);
}

RTMI_EXPORT int rtmi_render_rays_ris(rtmi_scene *s, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first, const double *rays,
                                     const uint64_t *keys, uint64_t seed, uint32_t ctr0, int32_t depth, int32_t n_lights, const int32_t *light_prims,
                                     double *state, double *out_mean, double *out_stderr, double *out_rays, uint64_t *out_counters) {
    return lit_rays_host(true, s, precision, n_groups, group, g_first, rays, keys, seed, ctr0, depth, n_lights, light_prims, 0, state, out_mean, out_stderr,
                         out_rays, out_counters, -1, true);
}

RTMI_EXPORT int rtmi_probe_paths_ris(rtmi_scene *s, int32_t precision, int32_t n, const double *rays, const uint64_t *keys, uint64_t ctr0, int32_t depth,
                                     int32_t n_lights, const int32_t *light_prims, double *out_rgb, uint64_t *out_nseg, double *out_weight, double *log,
                                     int32_t max_seg, int32_t *out_nlog) {
    return lit_probe(true, s, precision, n, rays, keys, ctr0, depth, n_lights, light_prims, 0, out_rgb, out_nseg, nullptr, out_weight, log, max_seg, out_nlog,
                     -1, true);
}

RTMI_EXPORT int rtmi_render_lit_ris_device(rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth,
                                           uint64_t seed, int32_t n_lights, const int32_t *light_prims, int32_t n_tiles, const void *d_tiles, void *d_state,
                                           void *d_out_linear, void *d_out_rgb8, void *d_out_stderr, void *d_out_rays, void *d_out_camera,
                                           void *d_out_counters, void *stream) {
    if (!d_tiles) return lit_frame_device(false, s, precision, nx, ny, s_first, s_count, depth, seed, 2, n_lights, light_prims, 0, d_state, d_out_linear,
                                          d_out_rgb8, d_out_stderr, d_out_rays, d_out_camera, d_out_counters, stream, true);
    return lit_tiles_device(s, precision, nx, ny, s_first, s_count, depth, seed, 2, n_lights, light_prims, 0, 0, n_tiles, d_tiles, d_state, d_out_linear,
                            d_out_rgb8, d_out_stderr, d_out_rays, d_out_camera, d_out_counters, stream, true);
}

RTMI_EXPORT int rtmi_render_lit_ris(rtmi_scene *s, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                                    int32_t n_lights, const int32_t *light_prims, int32_t n_tiles, const int32_t *tiles, double *state, double *out_linear,
                                    uint8_t *out_rgb8, double *out_stderr, double *out_rays, double *out_camera, uint64_t *out_counters) {
    if (!tiles) return lit_frame_host(false, s, precision, nx, ny, s_first, s_count, depth, seed, 2, n_lights, light_prims, 0, state, out_linear, out_rgb8,
                                      out_stderr, out_rays, out_camera, out_counters, true);
    return lit_tiles_host(s, precision, nx, ny, s_first, s_count, depth, seed, 2, n_lights, light_prims, 0, 0, n_tiles, tiles, state, out_linear, out_rgb8,
                          out_stderr, out_rays, out_camera, out_counters, true);
}

// ---- retiring the tiles of a caller's list by a noise map (rtmi_tiles_retire*): the stateless rtmi_adaptive_retire ------------------------------------------
// adaptive_retire_kernel over the caller's list with the whole image as the region, then adaptive_compact_kernel into the context's workspace (so the output
// may be the input), whose survivors go to the caller once their number is known.
namespace {
int check_tiles_retire_args(int nx, int ny, const void *noise, double eps, int n_tiles, const void *tiles_in, const void *tiles_out, const int32_t *out_count) {
    const int rc = check_retire_args(nx, ny, noise, eps);
    if (rc) return rc;
    if (n_tiles < 0 || (n_tiles > 0 && (!tiles_in || !tiles_out)) || !out_count)
        return fail(RTMI_E_ARG, "n_tiles must be >= 0 and tiles_in, tiles_out, out_count not NULL (got n_tiles = %d)", n_tiles);
    return RTMI_OK;
}

// d_noise and d_in are device pointers; the survivors lie in *d_kept behind the one synchronisation of `st`
int tiles_retire_impl(rtmi_ctx *c, int nx, int ny, const double *d_noise, double eps, int n, const int *d_in, int **d_kept, int32_t *out_count, hipStream_t st) {
    const int rc = c->retire_ws.ensure(((size_t)3 * (size_t)n + 2) * sizeof(int));
    if (rc) return rc;
    int *keep = reinterpret_cast<int *>(c->retire_ws.p), *kept = keep + n, *slots = kept + n, *d_meta = slots + n;
    hipLaunchKernelGGL(adaptive_retire_kernel, dim3((unsigned)(((long long)n * 64 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, d_noise, d_in, n, tiles_x_of(nx), nx,
                       0, 0, nx, ny, eps, keep);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(adaptive_compact_kernel, dim3(1), dim3(kCompactBlock), 0, st, keep, d_in, nullptr, n, kept, slots, d_meta, -1, nullptr, tiles_x_of(nx), 0, 0,
                       nx, ny);
    HIP_TRY(hipGetLastError());
    int meta[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(meta, d_meta, sizeof meta, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out_count = meta[0];
    *d_kept = kept;
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_tiles_retire_device(rtmi_ctx *c, int32_t nx, int32_t ny, const void *d_noise, double eps, int32_t n_tiles, const void *d_tiles_in,
                                         void *d_tiles_out, int32_t *out_count, void *stream) {
    int rc = check_tiles_retire_args(nx, ny, d_noise, eps, n_tiles, d_tiles_in, d_tiles_out, out_count);
    if (rc) return rc;
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    *out_count = 0;
    if (n_tiles == 0) return RTMI_OK;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    int *kept = nullptr;
    rc = tiles_retire_impl(c, nx, ny, as<const double>(d_noise), eps, n_tiles, as<const int>(d_tiles_in), &kept, out_count, st);
    if (rc || *out_count == 0) return rc;
    HIP_TRY(hipMemcpyAsync(d_tiles_out, kept, (size_t)*out_count * sizeof(int), hipMemcpyDeviceToDevice, st)); // in stream order: ahead of the caller's next call
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_tiles_retire(rtmi_ctx *c, int32_t nx, int32_t ny, const double *noise, double eps, int32_t n_tiles, const int32_t *tiles_in,
                                  int32_t *tiles_out, int32_t *out_count) {
    int rc = check_tiles_retire_args(nx, ny, noise, eps, n_tiles, tiles_in, tiles_out, out_count);
    if (rc) return rc;
    const int n_frame_tiles = tiles_x_of(nx) * tiles_x_of(ny);
    for (int k = 0; k < n_tiles; ++k)
        if (tiles_in[k] < 0 || tiles_in[k] >= n_frame_tiles) return fail(RTMI_E_ARG, "tiles_in[%d] = %d, the frame has %d tiles", k, tiles_in[k], n_frame_tiles);
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    *out_count = 0;
    if (n_tiles == 0) return RTMI_OK;
    HIP_TRY(hipSetDevice(c->device));
    HostIo io(c);
    double *d_noise;
    int *d_in;
    io.in(&d_noise, (size_t)nx * (size_t)ny, noise); io.in(&d_in, (size_t)n_tiles, tiles_in);
    rc = io.stage();
    if (rc) return rc;
    int *kept = nullptr;
    rc = tiles_retire_impl(c, nx, ny, d_noise, eps, n_tiles, d_in, &kept, out_count, c->stream);
    if (rc || *out_count == 0) return rc;
    HIP_TRY(hipMemcpy(tiles_out, kept, (size_t)*out_count * sizeof(int), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ---- light-sampled frames on several GPUs (rtmi_lit_tiles_records_device, rtmi_multi_lit_*): THE DEALT LIT FRAME of rtmi.h ---------------------------------
// The sample path is rtmi_render_lit_tiles_device's (rtmi_render_lit_ris_device's for the proposal rule) on every replica's own list, the decision
// rtmi_tiles_retire_device's; lit_tiles_record_kernel packs a replica's dealt tiles into the record of the dealt progressive frames, and the gather, the
// assemble and the counter sums behind it are those frames' (enqueue_gather, assemble_progressive_kernel, sum_counters_kernel).
RTMI_EXPORT int rtmi_lit_tiles_records_device(rtmi_ctx *c, int32_t nx, int32_t ny, int32_t tile_first, int32_t tile_stride, int32_t n_slots, const void *d_state,
                                              const void *d_linear, const void *d_stderr, void *d_out_rec, void *stream) {
    if (nx <= 0 || ny <= 0 || (long long)nx * ny > (1ll << 30)) return fail(RTMI_E_ARG, "nx, ny must be > 0 and the frame at most 2^30 pixels (got %d %d)", nx, ny);
    if (tile_first < 0 || tile_stride <= 0) return fail(RTMI_E_ARG, "tile_first must be >= 0 and tile_stride > 0 (got %d, %d)", tile_first, tile_stride);
    if (n_slots < 0 || n_slots > (1 << 24)) return fail(RTMI_E_ARG, "n_slots must be in [0, 2^24] (got %d)", n_slots);
    if (n_slots > 0 && (!d_state || !d_linear || !d_stderr || !d_out_rec)) return fail(RTMI_E_ARG, "d_state, d_linear, d_stderr or d_out_rec is NULL");
    if (!ctx_ok(c)) return fail(RTMI_E_STATE, "invalid context handle");
    if (n_slots == 0) return RTMI_OK;
    HIP_TRY(hipSetDevice(c->device));
    const long long npx = (long long)n_slots * 64;
    hipLaunchKernelGGL(lit_tiles_record_kernel, dim3((unsigned)((npx + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream_of(c, stream), as<const double>(d_state),
                       as<const double>(d_linear), as<const double>(d_stderr), tile_first, tile_stride, tiles_x_of(nx), tiles_x_of(nx) * tiles_y_of(ny), nx, ny,
                       n_slots, as<double>(d_out_rec));
    HIP_TRY(hipGetLastError());
    return RTMI_OK;
}

namespace {
// What the first render after create / reset fixes: a later render continues the frame only under the same key.
struct LitKey {
    int precision = 0, depth = 0, estimator = 0, volume = 0, light_choice = 0, n_lights = -1; // n_lights -1: no list (the scene's eligible lights)
    uint64_t seed = 0;
    std::vector<int32_t> lights;
    std::vector<uint64_t> revisions; // of the replicas' scenes
    bool operator==(const LitKey &o) const {
        return precision == o.precision && depth == o.depth && estimator == o.estimator && volume == o.volume && light_choice == o.light_choice &&
               n_lights == o.n_lights && seed == o.seed && lights == o.lights && revisions == o.revisions;
    }
    std::string text() const {
        char b[192];
        snprintf(b, sizeof b, "precision %d, depth %d, seed %llu, estimator %d, volume %d, light_choice %d, lights ", precision, depth, (unsigned long long)seed,
                 estimator, volume, light_choice);
        std::string s = b;
        if (n_lights < 0) s += "NULL";
        else { s += "["; for (size_t i = 0; i < lights.size(); ++i) s += (i ? " " : "") + std::to_string(lights[i]); s += "]"; }
        s += ", scene revisions [";
        for (size_t i = 0; i < revisions.size(); ++i) s += (i ? " " : "") + std::to_string((unsigned long long)revisions[i]);
        return s + "]";
    }
};

struct MultiLitReplica {
    DevBuf state, lin, se, tiles, rec, noise; // whole-frame state and planes, the active list, the record (replicas > 0), a caller's map (replicas > 0)
    std::vector<int32_t> owned;               // the dealing: tiles r, r + n, ..., ascending
    int n_active = 0;
};

struct MultiLitFrame {
    int n = 0, nx = 0, ny = 0, n_tiles = 0, per = 0, k = 0;
    bool keyed = false;
    LitKey key;
    std::vector<rtmi_scene *> scenes;
    std::vector<MultiLitReplica> rep;
    DevBuf gathered; // on replica 0's device: the records of all replicas, replica 0's in place
    size_t tile_words() const { return (size_t)per * 64 * RTMI_PROG_REC; }
    size_t rec_words() const { return tile_words() + 4; } // the tiles, then the call's four counters
};

std::map<uint64_t, std::unique_ptr<MultiLitFrame>> g_lit_frames; // by handle (never 0); under g_multi_mu
uint64_t g_lit_next = 1;

int lit_frame_of(uint64_t handle, MultiLitFrame **f) {
    if (handle == 0) return fail(RTMI_E_ARG, "frame is NULL");
    const auto it = g_lit_frames.find(handle);
    if (it == g_lit_frames.end()) return fail(RTMI_E_STATE, "invalid frame handle (destroyed, or never created)");
    *f = it->second.get();
    for (int r = 0; r < (*f)->n; ++r)
        if (!scene_ok((*f)->scenes[(size_t)r])) return fail(RTMI_E_STATE, "replica %d's scene was destroyed under the frame", r);
    return RTMI_OK;
}

void multi_lit_free(MultiLitFrame &f) {
    for (int r = 0; r < f.n; ++r) {
        MultiLitReplica &p = f.rep[(size_t)r];
        if (scene_ok(f.scenes[(size_t)r])) { (void)hipSetDevice(f.scenes[(size_t)r]->ctx->device); (void)hipStreamSynchronize(f.scenes[(size_t)r]->ctx->stream); }
        p.state.release(); p.lin.release(); p.se.release(); p.tiles.release(); p.rec.release(); p.noise.release();
        if (r == 0) f.gathered.release();
    }
}

// k = 0, every tile listed on its owner, the state's counts zero; waits for every replica's stream first
int multi_lit_reset(MultiLitFrame &f) {
    for (int r = 0; r < f.n; ++r) {
        MultiLitReplica &p = f.rep[(size_t)r];
        rtmi_ctx *c = f.scenes[(size_t)r]->ctx;
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (!p.owned.empty()) HIP_TRY(hipMemcpy(p.tiles.p, p.owned.data(), p.owned.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemsetAsync(p.state.p, 0, p.state.bytes, c->stream)); // (the context's stream is not ordered with the null stream)
        HIP_TRY(hipStreamSynchronize(c->stream));
        p.n_active = (int)p.owned.size();
        c->consume_pending = false;
    }
    f.k = 0; f.keyed = false;
    return RTMI_OK;
}

// the argument checks of a render that need no frame, in the header's order
int check_multi_lit_args(int precision, int s_count, int depth, int estimator, int light_choice, int volume) {
    if (s_count <= 0 || depth < 0) return fail(RTMI_E_ARG, "s_count must be > 0 and depth >= 0 (got %d, %d)", s_count, depth);
    if (estimator < 0 || estimator > 3) return fail(RTMI_E_ARG, "estimator must be 0 (plain), 1 (the NEE rule), 2 (the MIS rule) or 3 (the proposal rule) (got %d)", estimator);
    if (volume != 0 && volume != 1) return fail(RTMI_E_ARG, "volume must be 0 or 1 (got %d)", volume);
    if (estimator == 3 && volume == 1) return fail(RTMI_E_ARG, "estimator 3 (the proposal rule) has no volume form");
    if (precision != RTMI_F64 && precision != RTMI_F32) return fail(RTMI_E_ARG, "precision must be RTMI_F64 or RTMI_F32");
    return RTMI_OK;
}

struct LitPrep { RisLightTable Rt; RaysFrame F; bool work = false; };

// d_out_*: on replica 0's device, each may be null.  Returns with every replica's stream synchronised.
int multi_lit_render_impl(MultiLitFrame &f, int precision, int s_count, int depth, uint64_t seed, int estimator, int n_lights, const int32_t *light_prims,
                          int light_choice, int volume, double *d_lin, unsigned char *d_q, double *d_se, int *d_smp, u64 *d_cnt) {
    const int n = f.n;
    const bool ris = estimator == 3;
    const int est = ris ? 2 : estimator, choice = estimator == 2 ? light_choice : 0;
    if (light_prims && (n_lights < 0 || n_lights > RTMI_DIRECT_MAX_LIGHTS)) return fail(RTMI_E_ARG, "n_lights must be in [0, %d] (got %d)", RTMI_DIRECT_MAX_LIGHTS, n_lights);
    if (estimator == 2 && light_choice != 0 && light_choice != 1) return fail(RTMI_E_ARG, "light_choice must be 0 (uniform) or 1 (by power) (got %d)", light_choice);
    // the key
    LitKey key;
    key.precision = precision; key.depth = depth; key.estimator = estimator; key.volume = volume; key.light_choice = choice; key.seed = seed;
    key.n_lights = light_prims ? n_lights : -1;
    if (light_prims) key.lights.assign(light_prims, light_prims + n_lights);
    for (int r = 0; r < n; ++r) key.revisions.push_back(f.scenes[(size_t)r]->revision);
    if (f.keyed && !(key == f.key))
        return fail(RTMI_E_STATE, "the frame holds %d samples under {%s}; this call's key is {%s}: rtmi_multi_lit_reset starts another frame", f.k, f.key.text().c_str(),
                    key.text().c_str());
    if ((long long)f.k + s_count > INT32_MAX) return fail(RTMI_E_ARG, "k + s_count = %d + %d overflows int32", f.k, s_count);
    // the sibling's checks on every replica, before the first launch
    std::vector<LitPrep> prep((size_t)n);
    for (int r = 0; r < n; ++r) {
        MultiLitReplica &p = f.rep[(size_t)r];
        LitPrep &q = prep[(size_t)r];
        const LitTileArgs tl{volume, p.n_active, nullptr, p.tiles.p};
        const int rc = lit_frame_begin(f.scenes[(size_t)r], precision, f.nx, f.ny, f.k, s_count, depth, est, n_lights, light_prims, choice, nullptr, p.lin.p, p.se.p,
                                       q.Rt.m, q.F, &q.work, volume == 1, &tl);
        if (rc) { const std::string why = g_err; return fail(rc, "replica %d: %s", r, why.c_str()); }
        if (q.work && ris) make_ris_rows(q.Rt);
    }
    GatherPlan plan;
    int rc = plan_gather(n, f.scenes.data(), plan);
    if (rc) return rc;
    rtmi_ctx *c0 = f.scenes[0]->ctx;
    char *gathered = reinterpret_cast<char *>(f.gathered.p);
    const size_t rec = f.rec_words(), tile_words = f.tile_words();
    // A failure from here on resets the frame on every replica once every touched stream is idle (some replicas hold the new samples, some do not).
    int launched = 0;
    auto bail = [&](int code) {
        const std::string keep = g_err;
        for (int r = 0; r < launched; ++r) { (void)hipSetDevice(f.scenes[(size_t)r]->ctx->device); (void)hipStreamSynchronize(f.scenes[(size_t)r]->ctx->stream); }
        (void)hipSetDevice(c0->device); (void)hipStreamSynchronize(c0->stream);
        (void)multi_lit_reset(f);
        g_err = keep;
        return code;
    };
#define HIP_BAIL(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return bail(fail(RTMI_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_))); } while (0)
    // 1. every replica, on its own context stream: the trace and the fold of its listed tiles, the record of its dealt tiles, the call's counters
    std::vector<char *> recs((size_t)n);
    for (int r = 0; r < n; ++r) {
        MultiLitReplica &p = f.rep[(size_t)r];
        LitPrep &q = prep[(size_t)r];
        rtmi_scene *s = f.scenes[(size_t)r];
        rtmi_ctx *cr = s->ctx;
        launched = r + 1;
        HIP_BAIL(hipSetDevice(cr->device));
        char *buf = recs[(size_t)r] = r == 0 ? gathered : reinterpret_cast<char *>(p.rec.p);
        if (cr->consume_pending) { // the previous call's copy out of this record (on replica 0's stream) must have read it
            HIP_BAIL(hipStreamWaitEvent(cr->stream, cr->ev_consumed, 0));
            cr->consume_pending = false;
        }
        u64 *cnt = reinterpret_cast<u64 *>(buf) + tile_words;
        if (q.work) {
            q.F.out_camera = nullptr; q.F.d_tiles = as<const int>(p.tiles.p); q.F.d_rgb8 = nullptr;
            rc = lit_frame_run(s, precision, f.nx, f.ny, f.k, s_count, depth, seed, est, q.Rt.m, q.F, as<double>(p.state.p), as<double>(p.lin.p), nullptr,
                               as<double>(p.se.p), nullptr, cnt, cr->stream, volume == 1, ris ? &q.Rt : nullptr);
            if (rc) return bail(rc);
        } else
            HIP_BAIL(hipMemsetAsync(cnt, 0, 4 * sizeof(u64), cr->stream)); // no tile listed here: nothing traced
        const long long npx = (long long)f.per * 64;
        hipLaunchKernelGGL(lit_tiles_record_kernel, dim3((unsigned)((npx + kBlock - 1) / kBlock)), dim3(kBlock), 0, cr->stream, as<const double>(p.state.p),
                           as<const double>(p.lin.p), as<const double>(p.se.p), r, n, tiles_x_of(f.nx), f.n_tiles, f.nx, f.ny, f.per, reinterpret_cast<double *>(buf));
        HIP_BAIL(hipGetLastError());
        if (!plan.use_rccl && r > 0) { rc = ensure_event(&cr->ev_done); if (rc) return bail(rc); HIP_BAIL(hipEventRecord(cr->ev_done, cr->stream)); }
    }
    // 2. ONE gather to replica 0's device (n = 1 without RTMI_MULTI_GATHER=rccl: nothing to move)
    rc = enqueue_gather(n, f.scenes.data(), plan, recs, gathered, rec);
    if (rc) return bail(rc);
    // 3. replica 0 un-tiles, quantises and sums the counters
    HIP_BAIL(hipSetDevice(c0->device));
    if (d_lin || d_q || d_se || d_smp) {
        const long long npx = (long long)f.nx * f.ny;
        hipLaunchKernelGGL(assemble_progressive_kernel, dim3((unsigned)((npx + kBlock - 1) / kBlock)), dim3(kBlock), 0, c0->stream,
                           reinterpret_cast<const double *>(gathered), n, rec, tiles_x_of(f.nx), f.nx, f.ny, d_lin, d_q, d_se, d_smp);
        HIP_BAIL(hipGetLastError());
    }
    if (d_cnt) { // the record ends with four counters: sum_counters_kernel sums two
        for (int h = 0; h < 2; ++h)
            hipLaunchKernelGGL(sum_counters_kernel, dim3(1), dim3(64), 0, c0->stream, reinterpret_cast<const u64 *>(gathered), n, rec, tile_words + 2 * (size_t)h,
                               d_cnt + 2 * h);
        HIP_BAIL(hipGetLastError());
    }
    // 4. every stream idle; replica 0 last: its stream carries the gather and the assemble
    for (int r = n - 1; r >= 0; --r) {
        rtmi_ctx *cr = f.scenes[(size_t)r]->ctx;
        HIP_BAIL(hipSetDevice(cr->device));
        HIP_BAIL(hipStreamSynchronize(cr->stream));
    }
#undef HIP_BAIL
    for (int r = 1; r < n; ++r) f.scenes[(size_t)r]->ctx->consume_pending = false; // replica 0's stream is idle: the copies out of the records are done
    if (!f.keyed) { f.key = key; f.keyed = true; }
    f.k += s_count;
    return RTMI_OK;
}

// d_noise: null (every replica's own stderr plane) or a whole-frame map on replica 0's device, complete on replica 0's context stream
int multi_lit_retire_impl(MultiLitFrame &f, const double *d_noise, const double *host_noise, double eps, int32_t *out_count) {
    const int n = f.n;
    const size_t map_bytes = (size_t)f.nx * (size_t)f.ny * sizeof(double);
    rtmi_ctx *c0 = f.scenes[0]->ctx;
    int total = 0, touched = 0;
    auto bail = [&](int code) {
        const std::string keep = g_err;
        for (int r = 0; r < touched; ++r) { (void)hipSetDevice(f.scenes[(size_t)r]->ctx->device); (void)hipStreamSynchronize(f.scenes[(size_t)r]->ctx->stream); }
        (void)multi_lit_reset(f);
        g_err = keep;
        return code;
    };
#define HIP_BAIL(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return bail(fail(RTMI_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_))); } while (0)
    if (d_noise || host_noise) { // the map goes to every replica first: every copy is enqueued on the stream that replica's decision runs on
        if (d_noise && n > 1) { // a caller's device map is complete on replica 0's stream: the other streams wait for that point of it
            HIP_TRY(hipSetDevice(c0->device));
            const int rc = ensure_event(&c0->ev_done); // (the gather records ev_done on replicas > 0 only)
            if (rc) return rc;
            HIP_TRY(hipEventRecord(c0->ev_done, c0->stream));
        }
        for (int r = 0; r < n; ++r) {
            MultiLitReplica &p = f.rep[(size_t)r];
            rtmi_ctx *cr = f.scenes[(size_t)r]->ctx;
            if (p.n_active == 0 || (d_noise && r == 0)) continue; // (replica 0 reads a device map where it lies, on the stream it is complete on)
            HIP_TRY(hipSetDevice(cr->device));
            const int rc = p.noise.ensure(map_bytes);
            if (rc) return rc;
            if (host_noise) HIP_TRY(hipMemcpyAsync(p.noise.p, host_noise, map_bytes, hipMemcpyHostToDevice, cr->stream)); // (the decision below waits for the stream)
            else {
                HIP_TRY(hipStreamWaitEvent(cr->stream, c0->ev_done, 0));
                if (cr->device == c0->device) HIP_TRY(hipMemcpyAsync(p.noise.p, d_noise, map_bytes, hipMemcpyDeviceToDevice, cr->stream));
                else HIP_TRY(hipMemcpyPeerAsync(p.noise.p, cr->device, d_noise, c0->device, map_bytes, cr->stream));
            }
        }
    }
    for (int r = 0; r < n; ++r) {
        MultiLitReplica &p = f.rep[(size_t)r];
        rtmi_ctx *cr = f.scenes[(size_t)r]->ctx;
        if (p.n_active == 0) continue;
        touched = r + 1;
        HIP_BAIL(hipSetDevice(cr->device));
        const double *map = !d_noise && !host_noise ? as<const double>(p.se.p) : (d_noise && r == 0) ? d_noise : as<const double>(p.noise.p);
        int *kept = nullptr;
        int32_t count = 0;
        const int rc = tiles_retire_impl(cr, f.nx, f.ny, map, eps, p.n_active, as<const int>(p.tiles.p), &kept, &count, cr->stream);
        if (rc) return bail(rc);
        if (count > 0) HIP_BAIL(hipMemcpyAsync(p.tiles.p, kept, (size_t)count * sizeof(int), hipMemcpyDeviceToDevice, cr->stream)); // ahead of the next render
        p.n_active = count;
        total += count;
    }
#undef HIP_BAIL
    *out_count = total;
    return RTMI_OK;
}

int check_multi_lit_retire(MultiLitFrame &f) {
    if (f.k == 0) return fail(RTMI_E_STATE, "the frame holds no samples to retire tiles by (rtmi_multi_lit_render first)");
    return RTMI_OK;
}
} // namespace

RTMI_EXPORT int rtmi_multi_lit_create(int32_t n, rtmi_scene *const *scenes, int32_t nx, int32_t ny, uint64_t *out_frame) {
    if (n < 1 || n > RTMI_MULTI_LIT_MAX || !scenes) return fail(RTMI_E_ARG, "n must be 1..%d and scenes non-NULL (got %d)", RTMI_MULTI_LIT_MAX, n);
    if (nx <= 0 || ny <= 0 || (long long)nx * ny > (1ll << 30)) return fail(RTMI_E_ARG, "nx, ny must be > 0 and the frame at most 2^30 pixels (got %d %d)", nx, ny);
    if (!out_frame) return fail(RTMI_E_ARG, "out_frame is NULL");
    for (int r = 0; r < n; ++r) {
        if (!scene_ok(scenes[r])) return fail(RTMI_E_STATE, "replica %d: invalid scene handle", r);
        for (int q = 0; q < r; ++q)
            if (scenes[q]->ctx == scenes[r]->ctx) return fail(RTMI_E_ARG, "replicas %d and %d share a context (a context is not re-entrant: one per replica)", q, r);
        if (scenes[r]->n_prims != scenes[0]->n_prims) return fail(RTMI_E_ARG, "replica %d is not a clone of replica 0", r);
    }
    std::lock_guard<std::mutex> lock(g_multi_mu);
    DeviceGuard guard;
    std::unique_ptr<MultiLitFrame> f(new MultiLitFrame);
    f->n = n; f->nx = nx; f->ny = ny;
    f->n_tiles = tiles_x_of(nx) * tiles_y_of(ny);
    f->per = (f->n_tiles + n - 1) / n; // every replica's record is padded to this many tiles
    f->scenes.assign(scenes, scenes + n);
    f->rep.resize((size_t)n);
    const size_t npx = (size_t)nx * (size_t)ny;
    int rc = RTMI_OK;
    for (int r = 0; r < n && !rc; ++r) {
        MultiLitReplica &p = f->rep[(size_t)r];
        for (int t = r; t < f->n_tiles; t += n) p.owned.push_back(t);
        if (hipSetDevice(scenes[r]->ctx->device) != hipSuccess) { rc = fail(RTMI_E_DEVICE, "hipSetDevice(%d) failed", scenes[r]->ctx->device); break; }
        rc = p.state.ensure(npx * RTMI_RAYS_REC * sizeof(double));
        if (!rc) rc = p.lin.ensure(npx * 3 * sizeof(double));
        if (!rc) rc = p.se.ensure(npx * sizeof(double));
        if (!rc) rc = p.tiles.ensure(std::max<size_t>(1, p.owned.size()) * sizeof(int32_t));
        if (!rc) rc = r == 0 ? f->gathered.ensure((size_t)n * f->rec_words() * 8) : p.rec.ensure(f->rec_words() * 8);
        hipStream_t st = scenes[r]->ctx->stream; // (reset below waits for it)
        if (!rc && (hipMemsetAsync(p.lin.p, 0, p.lin.bytes, st) != hipSuccess || hipMemsetAsync(p.se.p, 0, p.se.bytes, st) != hipSuccess))
            rc = fail(RTMI_E_DEVICE, "hipMemset of replica %d's planes failed", r);
    }
    if (!rc) rc = multi_lit_reset(*f);
    if (rc) { const std::string keep = g_err; multi_lit_free(*f); g_err = keep; return rc; }
    *out_frame = g_lit_next++;
    g_lit_frames[*out_frame] = std::move(f);
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_multi_lit_destroy(uint64_t frame) {
    std::lock_guard<std::mutex> lock(g_multi_mu);
    if (frame == 0) return fail(RTMI_E_ARG, "frame is NULL");
    const auto it = g_lit_frames.find(frame);
    if (it == g_lit_frames.end()) return fail(RTMI_E_STATE, "invalid frame handle (destroyed, or never created)");
    DeviceGuard guard;
    multi_lit_free(*it->second);
    g_lit_frames.erase(it);
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_multi_lit_render_device(uint64_t frame, int32_t precision, int32_t s_count, int32_t depth, uint64_t seed, int32_t estimator, int32_t n_lights,
                                             const int32_t *light_prims, int32_t light_choice, int32_t volume, void *d_out_linear, void *d_out_rgb8,
                                             void *d_out_stderr, void *d_out_samples, void *d_out_counters) {
    if (frame == 0) return fail(RTMI_E_ARG, "frame is NULL");
    int rc = check_multi_lit_args(precision, s_count, depth, estimator, light_choice, volume);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(g_multi_mu);
    MultiLitFrame *f = nullptr;
    rc = lit_frame_of(frame, &f);
    if (rc) return rc;
    DeviceGuard guard;
    return multi_lit_render_impl(*f, precision, s_count, depth, seed, estimator, n_lights, light_prims, light_choice, volume, as<double>(d_out_linear),
                                 as<unsigned char>(d_out_rgb8), as<double>(d_out_stderr), as<int>(d_out_samples), as<u64>(d_out_counters));
}

RTMI_EXPORT int rtmi_multi_lit_render(uint64_t frame, int32_t precision, int32_t s_count, int32_t depth, uint64_t seed, int32_t estimator, int32_t n_lights,
                                      const int32_t *light_prims, int32_t light_choice, int32_t volume, double *out_linear, uint8_t *out_rgb8,
                                      double *out_stderr, int32_t *out_samples, uint64_t *out_counters) {
    if (frame == 0) return fail(RTMI_E_ARG, "frame is NULL");
    int rc = check_multi_lit_args(precision, s_count, depth, estimator, light_choice, volume);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(g_multi_mu);
    MultiLitFrame *f = nullptr;
    rc = lit_frame_of(frame, &f);
    if (rc) return rc;
    DeviceGuard guard;
    rtmi_ctx *c0 = f->scenes[0]->ctx;
    HIP_TRY(hipSetDevice(c0->device));
    const size_t npx = (size_t)f->nx * (size_t)f->ny;
    HostIo io(c0);
    double *d_lin, *d_se;
    unsigned char *d_q;
    int *d_smp;
    u64 *d_cnt;
    io.out(&d_lin, npx * 3, out_linear); io.out(&d_se, npx, out_stderr); io.out(&d_smp, npx, out_samples); io.out(&d_cnt, 4, out_counters);
    io.out(&d_q, npx * 3, out_rgb8);
    rc = io.reserve();
    if (rc) return rc;
    rc = multi_lit_render_impl(*f, precision, s_count, depth, seed, estimator, n_lights, light_prims, light_choice, volume, d_lin, d_q, d_se, d_smp, d_cnt);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c0->device)); // (every replica's stream is synchronised)
    const hipError_t e = io.download();
    if (e != hipSuccess) {
        (void)multi_lit_reset(*f);
        return fail(RTMI_E_DEVICE, "multi-device lit render: %s", hipGetErrorString(e));
    }
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_multi_lit_retire_device(uint64_t frame, const void *d_noise, double eps, int32_t *out_count) {
    if (frame == 0) return fail(RTMI_E_ARG, "frame is NULL");
    if (!(eps >= 0.0) || std::isinf(eps)) return fail(RTMI_E_ARG, "eps must be a finite number >= 0 (got %g)", eps);
    if (!out_count) return fail(RTMI_E_ARG, "out_count is NULL");
    std::lock_guard<std::mutex> lock(g_multi_mu);
    MultiLitFrame *f = nullptr;
    int rc = lit_frame_of(frame, &f);
    if (!rc) rc = check_multi_lit_retire(*f);
    if (rc) return rc;
    DeviceGuard guard;
    return multi_lit_retire_impl(*f, as<const double>(d_noise), nullptr, eps, out_count);
}

RTMI_EXPORT int rtmi_multi_lit_retire(uint64_t frame, const double *noise, double eps, int32_t *out_count) {
    if (frame == 0) return fail(RTMI_E_ARG, "frame is NULL");
    if (!(eps >= 0.0) || std::isinf(eps)) return fail(RTMI_E_ARG, "eps must be a finite number >= 0 (got %g)", eps);
    if (!out_count) return fail(RTMI_E_ARG, "out_count is NULL");
    std::lock_guard<std::mutex> lock(g_multi_mu);
    MultiLitFrame *f = nullptr;
    int rc = lit_frame_of(frame, &f);
    if (!rc) rc = check_multi_lit_retire(*f);
    if (rc) return rc;
    DeviceGuard guard;
    return multi_lit_retire_impl(*f, nullptr, noise, eps, out_count);
}

RTMI_EXPORT int rtmi_multi_lit_status(uint64_t frame, int32_t *out_k, int32_t *out_active) {
    std::lock_guard<std::mutex> lock(g_multi_mu);
    MultiLitFrame *f = nullptr;
    const int rc = lit_frame_of(frame, &f);
    if (rc) return rc;
    int active = 0;
    for (const MultiLitReplica &p : f->rep) active += p.n_active;
    if (out_k) *out_k = f->k;
    if (out_active) *out_active = active;
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_multi_lit_active_tiles(uint64_t frame, int32_t capacity, int32_t *out_tiles, int32_t *out_count) {
    if (frame == 0) return fail(RTMI_E_ARG, "frame is NULL");
    if (capacity < 0 || (capacity > 0 && !out_tiles) || !out_count) return fail(RTMI_E_ARG, "capacity must be >= 0 and out_tiles, out_count not NULL (got %d)", capacity);
    std::lock_guard<std::mutex> lock(g_multi_mu);
    MultiLitFrame *f = nullptr;
    const int rc = lit_frame_of(frame, &f);
    if (rc) return rc;
    DeviceGuard guard;
    std::vector<int32_t> all;
    for (int r = 0; r < f->n; ++r) {
        const MultiLitReplica &p = f->rep[(size_t)r];
        if (p.n_active == 0) continue;
        rtmi_ctx *c = f->scenes[(size_t)r]->ctx;
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const size_t at = all.size();
        all.resize(at + (size_t)p.n_active);
        HIP_TRY(hipMemcpy(all.data() + at, p.tiles.p, (size_t)p.n_active * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    std::sort(all.begin(), all.end()); // the replicas' lists are ascending and disjoint: the merge
    *out_count = (int32_t)all.size();
    if ((size_t)capacity < all.size()) return fail(RTMI_E_ARG, "capacity %d, the frame lists %zu tiles (*out_count holds the number)", capacity, all.size());
    std::copy(all.begin(), all.end(), out_tiles);
    return RTMI_OK;
}

RTMI_EXPORT int rtmi_multi_lit_reset(uint64_t frame) {
    std::lock_guard<std::mutex> lock(g_multi_mu);
    MultiLitFrame *f = nullptr;
    const int rc = lit_frame_of(frame, &f);
    if (rc) return rc;
    DeviceGuard guard;
    return multi_lit_reset(*f);
}
