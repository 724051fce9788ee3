// scene_build.h -- host half of scene creation that needs no device: the trees (BVH, entry grid, media neighbourhoods), the
// build team, and pack_scene, which turns the caller's arrays into the host copies of every device table.  No HIP runtime
// call and no kernel lives here; rtmi.hip includes it once, in its host section, and uploads what pack_scene returns.
// (It relies on the standard headers and on rtmi.h / rtmi_device.h as rtmi.hip includes them.)
#pragma once
#include <unistd.h> // getpid (the team below must not be used by a forked child)

namespace {

// The build's environment knobs, read once at the start of each scene creation (and of rtmi_test_build_tree).
struct BuildKnobs {
    int sah_levels = 1 << 20; // RTMI_BVH_SAH_LEVELS: number of top levels split by SAH (median below)
    int sweep_max = 0;        // RTMI_BVH_SWEEP_MAX: subtrees up to this many primitives take the exact sweep SAH
    double min_frac = 0.0;    // RTMI_BVH_MIN_FRAC: smallest share of a node's primitives a child may get
    bool grid_off = false;    // RTMI_GRID=0: no entry grid
    int grid_side = 0;        // RTMI_GRID=n (n > 1): n x n cells
    int grid_kmax = 4;        // RTMI_GRID_KMAX
    bool grid_walk = true;    // RTMI_GRID_WALK=0: the grid without the piecewise walk (tests)
    bool mloc = false;        // RTMI_MLOC=1: neighbourhood trees of the media
    int node16 = -1;          // RTMI_NODE16: 0 / 1 forces the node format, -1 chooses by area
    bool box_leaf = false;    // RTMI_BOX_LEAF=1: one leaf for the six faces of a Box
    bool small_scan = true;   // RTMI_SMALL_SCAN=0: no small-scene scan
    bool debug = false;       // RTMI_DEBUG: build timings and tree sizes on stderr
};
inline BuildKnobs read_build_knobs() {
    BuildKnobs k;
    if (const char *e = std::getenv("RTMI_BVH_SAH_LEVELS")) k.sah_levels = std::atoi(e);
    if (const char *e = std::getenv("RTMI_BVH_SWEEP_MAX")) k.sweep_max = std::atoi(e);
    if (const char *e = std::getenv("RTMI_BVH_MIN_FRAC")) k.min_frac = std::atof(e);
    if (const char *e = std::getenv("RTMI_GRID")) { k.grid_off = e[0] == '0'; k.grid_side = std::atoi(e); }
    if (const char *e = std::getenv("RTMI_GRID_KMAX")) k.grid_kmax = std::max(1, std::min(4, std::atoi(e)));
    if (const char *e = std::getenv("RTMI_GRID_WALK")) k.grid_walk = e[0] != '0';
    if (const char *e = std::getenv("RTMI_MLOC")) k.mloc = e[0] == '1';
    if (const char *e = std::getenv("RTMI_NODE16")) k.node16 = e[0] == '1';
    if (const char *e = std::getenv("RTMI_BOX_LEAF")) k.box_leaf = e[0] == '1';
    if (const char *e = std::getenv("RTMI_SMALL_SCAN")) k.small_scan = e[0] != '0';
    k.debug = std::getenv("RTMI_DEBUG") != nullptr;
    return k;
}

// ---- RTMI_ACCEL_BVH host build ----------------------------------------------------------------------------------------
// Binned-SAH binary BVH over the primitives' boxes, one primitive per leaf, each node carrying its two children's boxes
// (one 64-byte fetch per step).  Boxes are FLOAT, rounded outward and inflated by 2^-21 * obound (see slab_hit): the
// traversal is only a conservative filter in front of the exact FP64 sphere test, so the tree's shape affects speed, never
// results.  Primitives whose radius is a large fraction of the scene (sky dome, ground) are kept out of the tree.
struct BvhBox { double lo[3], hi[3]; };
struct BvhItem { BvhBox b; double cen[3]; int idx; };

inline void box_grow(BvhBox &a, const BvhBox &b) { for (int k = 0; k < 3; ++k) { a.lo[k] = std::min(a.lo[k], b.lo[k]); a.hi[k] = std::max(a.hi[k], b.hi[k]); } }
inline BvhBox box_empty() { BvhBox b; for (int k = 0; k < 3; ++k) { b.lo[k] = 1e300; b.hi[k] = -1e300; } return b; }
inline double box_area(const BvhBox &b) { const double x = b.hi[0] - b.lo[0], y = b.hi[1] - b.lo[1], z = b.hi[2] - b.lo[2]; return x < 0 ? 0.0 : 2.0 * (x * y + y * z + z * x); }
inline float f_down(double x) { float f = (float)x; if ((double)f > x) f = std::nextafterf(f, -INFINITY); return f; }
inline float f_up(double x) { float f = (float)x; if ((double)f < x) f = std::nextafterf(f, INFINITY); return f; }

// Host-side scene preparation (the device's trees) runs on a small TEAM of threads created once per process and kept: on the GPU boxes of this pool creating a
// thread costs ~0.3 ms, a team of 16 per call cost more than the 11 025 rectangle trees it built.  run(fn): the caller and every worker execute fn() once.
static std::atomic<int> g_build_single{0}; // test hook (rtmi_test_build_tree): build on the calling thread only
inline unsigned team_size() {
    unsigned n = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    if (const char *e = std::getenv("RTMI_BUILD_THREADS")) n = (unsigned)std::max(1, std::min(64, std::atoi(e)));
    return n;
}
inline unsigned build_threads() { return g_build_single.load() ? 1u : team_size(); }
class WorkTeam {
    std::vector<std::thread> th;
    std::mutex mu, use_mu;
    std::condition_variable cv, done_cv;
    const std::function<void()> *fn = nullptr;
    unsigned long gen = 0;
    unsigned pending = 0;
    bool stop = false;
    pid_t owner;
    void loop() {
        unsigned long seen = 0;
        for (;;) {
            const std::function<void()> *f;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || gen != seen; });
                if (stop) return;
                seen = gen; f = fn;
            }
            (*f)();
            { std::lock_guard<std::mutex> lk(mu); if (--pending == 0) done_cv.notify_all(); }
        }
    }
public:
    explicit WorkTeam(unsigned n) : owner(getpid()) { for (unsigned t = 1; t < n; ++t) th.emplace_back([this] { loop(); }); }
    ~WorkTeam() { { std::lock_guard<std::mutex> lk(mu); stop = true; } cv.notify_all(); for (std::thread &t : th) t.join(); }
    // one team per process, never destroyed (its threads wait on the condition variable until the process exits: no join in a static destructor, which a host
    // that unloads libraries in its own order -- a JVM, an interpreter -- could run while they still wait); a forked child has the object but not the threads
    static WorkTeam &get() { static WorkTeam *team = new WorkTeam(team_size()); return *team; }
    void run(const std::function<void()> &f) {
        std::unique_lock<std::mutex> use(use_mu, std::try_to_lock);
        if (!use.owns_lock() || th.empty() || g_build_single.load() || getpid() != owner) { f(); return; } // the team is busy with another host thread's scene: this one builds alone
        { std::lock_guard<std::mutex> lk(mu); fn = &f; pending = (unsigned)th.size(); ++gen; }
        cv.notify_all();
        f();
        std::unique_lock<std::mutex> lk(mu);
        done_cv.wait(lk, [&] { return pending == 0; });
    }
};
// fn(begin, end) over [0, n) in blocks taken from a shared counter; `first` (optional) is one more job some thread of the team takes before the blocks
template <typename F> void parallel_blocks(size_t n, size_t block, F fn, const std::function<void()> *first = nullptr) {
    std::atomic<size_t> next{0};
    std::atomic<bool> first_taken{first == nullptr};
    const std::function<void()> worker = [&]() {
        if (!first_taken.exchange(true)) (*first)();
        for (size_t b = next.fetch_add(block); b < n; b = next.fetch_add(block)) fn(b, std::min(n, b + block));
    };
    if (n < 4 * block && !first) { worker(); return; }
    WorkTeam::get().run(worker);
}
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct BvhBuilder {
    std::vector<BvhItem> items;
    std::vector<float> nodes; // 16 floats per node
    std::vector<char> moving; // by original primitive index
    std::vector<char> box6;   // by original primitive index: the first of six rectangles that form a Box (one leaf: RTMI_LEAF_BOX)
    double delta = 0.0;
    const BvhBuilder *flags = nullptr; // a per-job builder (entry-grid rectangle trees) reads the flag vectors of the scene's builder instead of copying them
    int leaf_code(int idx) const {
        const BvhBuilder &f = flags ? *flags : *this;
        return ~(idx | (f.moving[(size_t)idx] ? 0x40000000 : 0) | (!f.box6.empty() && f.box6[(size_t)idx] ? RTMI_LEAF_BOX : 0));
    }
    int sah_depth = 8, max_depth = 0;
    double min_frac = 0.0;    // experiments: RTMI_BVH_MIN_FRAC = smallest share of a node's primitives a child may get (balance)
    int sweep_max = 0;  // subtrees up to this many primitives: exact sweep SAH; above: 32 bins (build time)
    int sah_levels = 1 << 20; // experiments: RTMI_BVH_SAH_LEVELS = number of top levels split by SAH (median below)
    BvhBox bounds(int b, int e) const { BvhBox r = box_empty(); for (int i = b; i < e; ++i) box_grow(r, items[(size_t)i].b); return r; }
    // node record (16 floats): l.lo.xy l.hi.xy | r.lo.xy r.hi.xy | l.lo.z l.hi.z r.lo.z r.hi.z | left, right, 0, 0
    void put_box(int node, int side, const BvhBox &b) {
        float *q = &nodes[(size_t)node * 16];
        for (int k = 0; k < 2; ++k) { q[side * 4 + k] = f_down(b.lo[k] - delta); q[side * 4 + 2 + k] = f_up(b.hi[k] + delta); }
        q[8 + side * 2] = f_down(b.lo[2] - delta); q[8 + side * 2 + 1] = f_up(b.hi[2] + delta);
    }
    void put_empty_box(int node, int side) {
        float *q = &nodes[(size_t)node * 16];
        for (int k = 0; k < 2; ++k) { q[side * 4 + k] = INFINITY; q[side * 4 + 2 + k] = -INFINITY; }
        q[8 + side * 2] = INFINITY; q[8 + side * 2 + 1] = -INFINITY;
    }
    int lone(const BvhItem &it) { // a tree over one primitive: a node whose right child is an empty box (a bare leaf code would skip the box test)
        const int node = (int)(nodes.size() / 16);
        nodes.resize(nodes.size() + 16, 0.0f);
        put_box(node, 0, it.b);
        put_empty_box(node, 1);
        const int l = leaf_code(it.idx);
        std::memcpy(&nodes[(size_t)node * 16 + 12], &l, 4); std::memcpy(&nodes[(size_t)node * 16 + 13], &l, 4);
        return node * 64;
    }
    int build(int b, int e, int depth) { // returns the child code of the subtree over items [b, e): byte offset of the node, or a leaf code
        max_depth = std::max(max_depth, depth);
        if (e - b == 1) return leaf_code(items[(size_t)b].idx);
        const int node = (int)(nodes.size() / 16);
        nodes.resize(nodes.size() + 16, 0.0f);
        // split: binned SAH (32 bins) over all three axes, the cheapest split wins; median split on the longest axis as the fallback
        // (also beyond sah_depth, to bound the stack)
        double clo[3] = {1e300, 1e300, 1e300}, chi[3] = {-1e300, -1e300, -1e300};
        for (int i = b; i < e; ++i) for (int k = 0; k < 3; ++k) { clo[k] = std::min(clo[k], items[(size_t)i].cen[k]); chi[k] = std::max(chi[k], items[(size_t)i].cen[k]); }
        int axis = 0;
        for (int k = 1; k < 3; ++k) if (chi[k] - clo[k] > chi[axis] - clo[axis]) axis = k;
        int mid = (b + e) / 2;
        bool done = false;
        // SAH wherever the subtree can still be finished by median splits within the stack's depth: depth + ceil(log2(count)) + 1
        // levels at most (a global cap on the SAH depth left the deep, crowded parts of large scenes to median splits)
        int lgc = 1;
        while ((1 << lgc) < e - b) ++lgc;
        if (depth + lgc + 1 < sah_depth && e - b > 2 && depth < sah_levels && e - b <= sweep_max) {
            // exact sweep SAH: for each axis sort by centroid, try every split position (suffix boxes, then one forward pass)
            double best = 1e300; int best_pos = -1;
            const int n = e - b;
            std::vector<BvhItem> tmp((size_t)n), best_order;
            std::vector<double> suffix((size_t)n + 1);
            for (int ax = 0; ax < 3; ++ax) {
                if (!(chi[ax] - clo[ax] > 0)) continue;
                std::copy(items.begin() + b, items.begin() + e, tmp.begin());
                std::sort(tmp.begin(), tmp.end(), [&](const BvhItem &x, const BvhItem &y) { return x.cen[ax] < y.cen[ax] || (x.cen[ax] == y.cen[ax] && x.idx < y.idx); });
                BvhBox acc = box_empty();
                for (int i = n - 1; i > 0; --i) { box_grow(acc, tmp[(size_t)i].b); suffix[(size_t)i] = box_area(acc); }
                acc = box_empty();
                bool improved = false;
                for (int i = 0; i < n - 1; ++i) { // left = [0, i], right = [i+1, n)
                    box_grow(acc, tmp[(size_t)i].b);
                    const double cost = box_area(acc) * (i + 1) + suffix[(size_t)i + 1] * (n - 1 - i);
                    if (std::min(i + 1, n - 1 - i) < min_frac * n) continue;
                    if (cost < best) { best = cost; best_pos = i + 1; improved = true; }
                }
                if (improved) best_order = tmp;
            }
            if (best_pos > 0) {
                std::copy(best_order.begin(), best_order.end(), items.begin() + b);
                mid = b + best_pos;
                done = true;
            }
        } else if (depth + lgc + 1 < sah_depth && e - b > 2 && depth < sah_levels) {
            const int NB = 32;
            double best = 1e300; int best_k = -1, best_axis = -1;
            for (int ax = 0; ax < 3; ++ax) {
                const double ext = chi[ax] - clo[ax];
                if (!(ext > 0)) continue;
                // Only OCCUPIED bins matter: between two occupied bins the two sides of a split -- boxes and counts -- do not change, so every split position of
                // such a run costs the same and the strict `cost < best` keeps the run's first, which is the occupied bin itself.  Walking the occupied bins (at
                // most e - b of them) instead of all 32 gives the same split for a fraction of the work on the small sets of the entry grid's rectangle trees
                // (3 - 14 primitives each, 11 025 trees at C3).
                BvhBox bb[NB]; int cnt[NB];
                unsigned occ = 0;
                for (int i = b; i < e; ++i) {
                    const int q = std::min(NB - 1, std::max(0, (int)((items[(size_t)i].cen[ax] - clo[ax]) / ext * NB)));
                    if (!((occ >> q) & 1u)) { bb[q] = box_empty(); cnt[q] = 0; occ |= 1u << q; }
                    box_grow(bb[q], items[(size_t)i].b); cnt[q]++;
                }
                int list[NB], m = 0;
                for (int q = 0; q < NB; ++q) if ((occ >> q) & 1u) list[m++] = q;
                BvhBox right[NB]; int rc[NB]; // right[j] / rc[j]: the occupied bins list[j], list[j + 1], ...
                BvhBox acc = box_empty(); int n = 0;
                for (int j = m - 1; j > 0; --j) { box_grow(acc, bb[list[j]]); n += cnt[list[j]]; right[j] = acc; rc[j] = n; }
                acc = box_empty(); n = 0;
                for (int j = 0; j + 1 < m; ++j) { // split after bin k = list[j]
                    box_grow(acc, bb[list[j]]); n += cnt[list[j]];
                    if (std::min(n, rc[j + 1]) < min_frac * (e - b)) continue;
                    const double cost = box_area(acc) * n + box_area(right[j + 1]) * rc[j + 1];
                    if (cost < best) { best = cost; best_k = list[j]; best_axis = ax; }
                }
            }
            if (best_k >= 0) {
                const double ext = chi[best_axis] - clo[best_axis], lo = clo[best_axis];
                auto it = std::partition(items.begin() + b, items.begin() + e, [&](const BvhItem &x) {
                    return std::min(NB - 1, std::max(0, (int)((x.cen[best_axis] - lo) / ext * NB))) <= best_k; });
                mid = (int)(it - items.begin());
                done = mid > b && mid < e;
            }
        }
        if (!done) {
            mid = (b + e) / 2;
            std::nth_element(items.begin() + b, items.begin() + mid, items.begin() + e,
                             [&](const BvhItem &x, const BvhItem &y) { return x.cen[axis] < y.cen[axis] || (x.cen[axis] == y.cen[axis] && x.idx < y.idx); });
        }
        const BvhBox lb = bounds(b, mid), rb = bounds(mid, e);
        const int l = build(b, mid, depth + 1);
        const int r = build(mid, e, depth + 1);
        put_box(node, 0, lb);
        put_box(node, 1, rb);
        std::memcpy(&nodes[(size_t)node * 16 + 12], &l, 4);
        std::memcpy(&nodes[(size_t)node * 16 + 13], &r, 4);
        return node * 64;
    }
};

// World-space box of primitive i in double (with a little slack): the local box of the innermost record, then each
// instance wrapper's outward map applied to its 8 corners, innermost wrapper first (RotateY: hitable.clj:441-443; Translate: 396).
// MovingSpheres: the sweep over the shutter interval.  Returns false when the primitive cannot be bounded.
bool prim_world_box(int kind, const double *g, const int32_t *xf_kind, const double *xf_param, int xf_first, int xf_count,
                    double t_lo, double t_hi, BvhBox &out) {
    BvhBox b;
    if (kind <= RTMI_PRIM_MOVING) {
        const double r = std::fabs(g[3]);
        if (kind == RTMI_PRIM_MOVING) {
            const double f0 = (t_lo - g[7]) / (g[8] - g[7]), f1 = (t_hi - g[7]) / (g[8] - g[7]);
            if (!std::isfinite(f0) || !std::isfinite(f1)) return false;
            for (int k = 0; k < 3; ++k) {
                const double a0 = g[k] * (1.0 - f0) + g[4 + k] * f0, a1 = g[k] * (1.0 - f1) + g[4 + k] * f1;
                b.lo[k] = std::min(a0, a1) - r; b.hi[k] = std::max(a0, a1) + r;
            }
        } else for (int k = 0; k < 3; ++k) { b.lo[k] = g[k] - r; b.hi[k] = g[k] + r; }
    } else if (kind <= RTMI_PRIM_RECT_YZ) {
        const int ax = kind == RTMI_PRIM_RECT_XY ? 2 : (kind == RTMI_PRIM_RECT_XZ ? 1 : 0);
        const int ua = kind == RTMI_PRIM_RECT_YZ ? 1 : 0, va = kind == RTMI_PRIM_RECT_XY ? 1 : 2;
        b.lo[ua] = std::min(g[0], g[2]); b.hi[ua] = std::max(g[0], g[2]);
        b.lo[va] = std::min(g[1], g[3]); b.hi[va] = std::max(g[1], g[3]);
        b.lo[ax] = g[4]; b.hi[ax] = g[4];
    } else {
        for (int k = 0; k < 3; ++k) { b.lo[k] = std::min(g[k], std::min(g[3 + k], g[6 + k])); b.hi[k] = std::max(g[k], std::max(g[3 + k], g[6 + k])); }
    }
    if ((kind == RTMI_PRIM_SPHERE || kind == RTMI_PRIM_UVSPHERE) && xf_count > 0) {
        // A sphere under Translate / RotateY wrappers is a sphere of the same radius about the mapped centre: its world box is centre +- r, not the box of the
        // eight rotated corners of its local box (a RotateY of 15 degrees grows that one by a fifth per side -- half again the area -- and make-final's
        // thousand spheres sit behind one).  The wrappers' own rounding moves a hit point by ~1e-13 of a coordinate; the slack below and the tree's 2^-21 obound cover it.
        double c[3] = {g[0], g[1], g[2]};
        const double r = std::fabs(g[3]);
        for (int q = xf_count - 1; q >= 0; --q) {
            const double *p = xf_param + (size_t)(xf_first + q) * 3;
            if (xf_kind[xf_first + q] == RTMI_XFORM_TRANSLATE) { c[0] += p[0]; c[1] += p[1]; c[2] += p[2]; }
            else { const double sn = p[0], cs = p[1]; const double rx = cs * c[0] + sn * c[2], rz = -(sn * c[0]) + cs * c[2]; c[0] = rx; c[2] = rz; }
        }
        for (int k = 0; k < 3; ++k) { const double pad = 1e-9 * (std::fabs(c[k]) + r) + 1e-12; b.lo[k] = c[k] - r - pad; b.hi[k] = c[k] + r + pad; }
    } else
    for (int q = xf_count - 1; q >= 0; --q) {
        const double *p = xf_param + (size_t)(xf_first + q) * 3;
        BvhBox nb = box_empty();
        for (int c = 0; c < 8; ++c) {
            double x = (c & 1) ? b.hi[0] : b.lo[0], y = (c & 2) ? b.hi[1] : b.lo[1], z = (c & 4) ? b.hi[2] : b.lo[2];
            if (xf_kind[xf_first + q] == RTMI_XFORM_TRANSLATE) { x += p[0]; y += p[1]; z += p[2]; }
            else { const double sn = p[0], cs = p[1]; const double rx = cs * x + sn * z, rz = -(sn * x) + cs * z; x = rx; z = rz; }
            const double pt[3] = {x, y, z};
            for (int k = 0; k < 3; ++k) { nb.lo[k] = std::min(nb.lo[k], pt[k]); nb.hi[k] = std::max(nb.hi[k], pt[k]); }
        }
        b = nb;
    }
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(b.lo[k]) || !std::isfinite(b.hi[k]) || std::fabs(b.lo[k]) > 1e15 || std::fabs(b.hi[k]) > 1e15) return false;
        const double slack = 1e-9 * (std::fabs(b.lo[k]) + std::fabs(b.hi[k])) + 1e-12;
        b.lo[k] -= slack; b.hi[k] += slack;
    }
    out = b;
    return true;
}

// the IEEE half at or beyond x in the given direction (up: >= x, else <= x); beyond the half range: +-inf.  Integer arithmetic on the float's bits (directed
// rounding of the magnitude: toward zero by truncation, away from zero by truncation + 1 when inexact): a host without F16C converts _Float16 in software, and a
// scene's tree has twelve planes per node (C3: 1.4 million conversions there and back).  rtmi_test_half_outward exposes it to the CPU test against numpy.
static uint16_t half_outward(float x, bool up) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    const uint32_t sign = u >> 31, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(0x7e00u | (sign << 15)); // NaN
    const bool away = up != (sign != 0); // the magnitude rounds away from zero
    uint32_t m;
    bool inexact;
    if (a >= 0x47800000u) { m = a == 0x7f800000u ? 0x7c00u : 0x7bffu; inexact = a != 0x7f800000u; } // >= 2^16: the largest half (65504) toward zero, inf away
    else if (a >= 0x38800000u) { m = (((a >> 23) - 112u) << 10) | ((a & 0x7fffffu) >> 13); inexact = (a & 0x1fffu) != 0; } // normal halves: 2^-14 <= |x| < 2^16
    else { const float sc = std::fabs(x) * 16777216.0f; m = (uint32_t)sc; inexact = (float)m != sc; } // half subnormals: units of 2^-24 (the scaling is exact)
    if (inexact && away) m += 1; // (carries into the exponent: 0x03ff + 1 = the smallest normal, 0x7bff + 1 = inf)
    return (uint16_t)(m | (sign << 15));
}
// What the trees of a scene were built with, kept by the scene: rtmi_scene_set_geometry judges an edit against it (never against a later edit).
enum { TB_ITEM = 1, TB_BIG = 2, TB_TALL = 4, TB_LAYER = 8, TB_UNBOUNDED = 16 };
struct TreeBuild {
    double obound = 0.0, cbound = 0.0, delta = 0.0; // unrounded (DevScene holds f_down(obound), f_up(cbound))
    std::vector<unsigned char> cls;                 // per world primitive: TB_* bits (tall / layer only where the entry grid was built)
    bool box_leaves = false;                        // a Box went into the tree as one leaf (RTMI_BOX_LEAF)
    bool grid = false;                              // the entry grid was built: lb .. cell hold
    BvhBox lb{}, tb{};                              // the layer's box, the tall primitives' box
    int G = 0;
    double csx = 0.0, csz = 0.0, eps = 0.0;
    std::vector<int> cell;                          // per world primitive: i0 i1 j0 j1, the cells a layer primitive was registered in
};
// the range of grid cells a layer primitive's box is registered in (build_bvh, and the displacement rule of rtmi_scene_set_geometry)
inline void grid_cell_range(const BvhBox &b, const BvhBox &lb, int G, double csx, double csz, double eps, int r[4]) {
    r[0] = std::max(0, std::min(G - 1, (int)std::floor((b.lo[0] - 2 * eps - lb.lo[0]) / csx))); r[1] = std::max(0, std::min(G - 1, (int)std::floor((b.hi[0] + 2 * eps - lb.lo[0]) / csx)));
    r[2] = std::max(0, std::min(G - 1, (int)std::floor((b.lo[2] - 2 * eps - lb.lo[2]) / csz))); r[3] = std::max(0, std::min(G - 1, (int)std::floor((b.hi[2] + 2 * eps - lb.lo[2]) / csz)));
}
// the box build_bvh gives a world primitive: its world box, or everything for one that cannot be bounded
inline BvhBox tree_item_box(bool bounded, const BvhBox &wbox) {
    if (bounded) return wbox;
    BvhBox b;
    for (int k = 0; k < 3; ++k) { b.lo[k] = -1e15; b.hi[k] = 1e15; }
    return b;
}
// fills d.bvh_* ; returns the node array to upload.  wbox[i] / bounded[i]: prim_world_box of every primitive.
// box_first[i] != 0: primitives i .. i + 5 are the six faces of one Box (detected at scene creation) -- one leaf, unless the box is too large for the tree
std::vector<float> build_bvh(DevScene &d, int n_prims, const int *prim_kind, const std::vector<BvhBox> &wbox, const std::vector<char> &bounded, const double *cam,
                             bool want_grid, std::vector<int> &grid_cells, const std::vector<char> &box_first, const BuildKnobs &K, int *out_depth = nullptr,
                             const std::vector<BvhBox> *media_boxes = nullptr, TreeBuild *rec = nullptr) {
    BvhBuilder B;
    struct DepthOut { BvhBuilder &b; int *o; ~DepthOut() { if (o) *o = b.max_depth; } } depth_out{B, out_depth};
    std::vector<BvhItem> all;
    double obound = 0.0;
    for (int k = 0; k < 3; ++k) obound = std::max(obound, std::fabs(cam[k]));
    for (int i = 0; i < n_prims; ++i) {
        if (prim_kind[i] == RTMI_PRIM_MEDIUM) continue; // media are not surfaces (ext_medium_test)
        BvhItem it; it.idx = i;
        if (bounded[(size_t)i]) {
            it.b = wbox[(size_t)i];
            for (int k = 0; k < 3; ++k) it.cen[k] = 0.5 * (it.b.lo[k] + it.b.hi[k]);
        } else { for (int k = 0; k < 3; ++k) { it.b.lo[k] = -1e15; it.b.hi[k] = 1e15; it.cen[k] = 0; } } // unbounded: goes to the big list below
        for (int k = 0; k < 3; ++k) obound = std::max(obound, std::max(std::fabs(it.b.lo[k]), std::fabs(it.b.hi[k])));
        all.push_back(it);
    }
    obound = std::min(obound, 1e15) * 1.001 + 1e-30;
    d.n_big = 0;
    B.box6.assign((size_t)std::max(n_prims, 1), 0);
    for (size_t a = 0; a < all.size(); ++a) {
        BvhItem it = all[a];
        if (!box_first.empty() && box_first[(size_t)it.idx] && a + 5 < all.size() && all[a + 5].idx == it.idx + 5) { // a Box: the union of its six faces, if that fits the tree
            BvhBox u = it.b;
            bool ok = bounded[(size_t)it.idx] != 0;
            for (int k = 1; k < 6; ++k) { box_grow(u, all[a + (size_t)k].b); ok = ok && bounded[(size_t)it.idx + (size_t)k]; }
            const double uext = std::max(u.hi[0] - u.lo[0], std::max(u.hi[1] - u.lo[1], u.hi[2] - u.lo[2]));
            if (ok && uext < 0.25 * obound) {
                it.b = u;
                for (int k = 0; k < 3; ++k) it.cen[k] = 0.5 * (u.lo[k] + u.hi[k]);
                B.box6[(size_t)it.idx] = 1;
                B.items.push_back(it);
                a += 5;
                continue;
            }
        }
        const double ext = std::max(it.b.hi[0] - it.b.lo[0], std::max(it.b.hi[1] - it.b.lo[1], it.b.hi[2] - it.b.lo[2]));
        if (ext >= 0.25 * obound && d.n_big < 16) d.big_idx[d.n_big++] = it.idx; // ascending index order
        else B.items.push_back(it);
    }
    B.delta = obound * (1.0 / 2097152.0); // 2^-21 * obound
    B.moving.assign((size_t)std::max(n_prims, 1), 0);
    for (int i = 0; i < n_prims; ++i) B.moving[(size_t)i] = prim_kind[i] == RTMI_PRIM_MOVING;
    d.bvh_obound = f_down(obound);
    double cbound = 0.0;
    for (const BvhItem &it : B.items) for (int k = 0; k < 3; ++k) cbound = std::max(cbound, std::max(std::fabs(it.b.lo[k]), std::fabs(it.b.hi[k])));
    d.bvh_cbound = f_up(cbound);
    if (rec) {
        *rec = TreeBuild();
        rec->obound = obound; rec->cbound = cbound; rec->delta = B.delta;
        rec->cls.assign((size_t)std::max(n_prims, 1), 0);
        rec->cell.assign((size_t)std::max(n_prims, 1) * 4, 0);
        for (int i = 0; i < n_prims; ++i) if (prim_kind[i] != RTMI_PRIM_MEDIUM && !bounded[(size_t)i]) rec->cls[(size_t)i] |= TB_UNBOUNDED;
        for (int k = 0; k < d.n_big; ++k) rec->cls[(size_t)d.big_idx[k]] |= TB_BIG;
        for (const BvhItem &it : B.items) rec->cls[(size_t)it.idx] |= TB_ITEM;
        for (char c : B.box6) rec->box_leaves = rec->box_leaves || c;
    }
    std::vector<BvhItem> grid_items;
    std::function<void()> whole_job; // the whole tree's build, when it is deferred to run beside the grid's jobs
    if (B.items.empty()) d.bvh_root = RTMI_BVH_EMPTY;
    else if (B.items.size() == 1) d.bvh_root = B.lone(B.items[0]);
    else {
        B.sah_levels = K.sah_levels; B.sweep_max = K.sweep_max; B.min_frac = K.min_frac;
        B.sah_depth = RTMI_BVH_STACK - 2; // depth budget: a node at depth d over k primitives may use SAH while d + ceil(log2 k) + 1 < budget
        // The whole tree and the entry grid's rectangle trees are independent: when a grid will be tried, the whole tree is built on a thread of its own
        // (into B.nodes, which the grid's jobs do not touch: they build into builders of their own and are appended after the join)
        grid_items.assign(B.items.begin(), B.items.end()); // (build() reorders B.items: the grid works on a copy taken before)
        auto build_whole = [&B, &d, &K]() {
            const double tb0 = now_ms();
            d.bvh_root = B.build(0, (int)B.items.size(), 0);
            if (K.debug) fprintf(stderr, "[rtmi] build: whole tree over %zu primitives %.2f ms\n", B.items.size(), now_ms() - tb0);
        };
        if (want_grid && B.items.size() >= 256 && build_threads() > 1) whole_job = build_whole; // deferred: the team's first job, beside the grid's rectangle trees
        else build_whole();
    }
    auto join_whole = [&]() {
        if (whole_job) { whole_job(); whole_job = nullptr; } // (no grid was built after all: build it here)
        if (d.bvh_root >= 0 && (B.max_depth >= RTMI_BVH_STACK - 1 || B.nodes.size() / 16 >= (1u << 25))) { // cannot happen by construction / node byte offsets are 31-bit
            d.bvh_root = RTMI_BVH_EMPTY; d.n_big = 0; d.bvh_obound = -1.0f; // obound < 0: every ray takes the exact flat scan
            B.nodes.clear();
        }
    };
    // ---- entry grid: a BVH per x-z cell over the primitives whose boxes overlap the cell (DevScene::grid_*) -------------------------------------
    d.grid_n = 0; d.grid_tall = RTMI_BVH_EMPTY; d.grid_kmax = 4; d.grid_walk = 0;
    grid_cells.clear();
    const double tg0 = now_ms();
    struct GridTimer { double t0; bool on; ~GridTimer() { if (on) fprintf(stderr, "[rtmi] build: entry grid + node formats %.2f ms\n", now_ms() - t0); } } grid_timer{tg0, K.debug};
    if (want_grid && !K.grid_off && grid_items.size() >= 256) { // (the whole tree may still be in the making: nothing below touches B.nodes / B.items before join_whole())
        const size_t n_items = grid_items.size();
        const std::vector<BvhItem> &world = grid_items; // (any order will do)
        // the layer: every primitive except the few much taller than the typical one (the cover scene's three big spheres among 10 000 small ones)
        std::vector<double> hts(n_items);
        for (size_t i = 0; i < n_items; ++i) hts[i] = world[i].b.hi[1] - world[i].b.lo[1];
        std::vector<double> sorted_h(hts);
        std::nth_element(sorted_h.begin(), sorted_h.begin() + (long)(n_items / 2), sorted_h.end());
        const double tall_h = 3.0 * sorted_h[n_items / 2] + 1e-300;
        std::vector<BvhItem> layer, tall;
        for (size_t i = 0; i < n_items; ++i) (hts[i] > tall_h ? tall : layer).push_back(world[i]);
        BvhBox lb = box_empty();
        for (const BvhItem &it : layer) box_grow(lb, it.b);
        const double ex = lb.hi[0] - lb.lo[0], ez = lb.hi[2] - lb.lo[2], ey = lb.hi[1] - lb.lo[1];
        // ~3.5 primitives per cell (C3: 53 x 53 cells, C2: 12 x 12).  Before long segments were walked in pieces (RTMI_GRID_CHUNK) ~10 per cell was best (C3, 16 .. 48
        // cells per side: 84.1 / 82.3 / 83.3 ms: a finer grid sent more rays to the root of the whole tree); with the walk 32 / 40 / 48 / 56 / 64 / 72 cells: 77.2 / 76.2 /
        // 76.4 / 76.1 / 76.7 / 78.5 ms, C2 7 / 10 / 14 / 20 cells: 3.39 / 3.37 / 3.33 / 3.49 ms
        // ... and cells no smaller than ~4.5 x the layer's height: a ray crosses the layer over a horizontal distance of height / tan(elevation), so a
        // taller layer (the moving cover scene: its spheres sweep up to 0.5 upwards, the layer is 0.9 instead of 0.4 high) at the same cell size means more
        // cells per segment, i.e. more pieces (C2 moving, 6 / 8 / 10 / 12 / 16 cells per side: 3.55 / 3.60 / 3.68 / 3.75 / 4.01 ms; for the static scenes both
        // rules give the same cell)
        int G = (int)std::lround(std::min(std::sqrt((double)layer.size() / 3.5), std::min(ex, ez) / (4.5 * std::max(ey, 1e-300))));
        if (K.grid_side > 1) G = K.grid_side;
        G = std::max(2, std::min(G, 256)); // (90 000 spheres: 160 x 160 cells)
        // worth it for a flat, wide layer of many primitives with few tall outliers
        if (layer.size() >= 256 && tall.size() * 20 <= n_items && ex > 0 && ez > 0 && ey < 0.25 * std::min(ex, ez)) {
            const double eps = 4.0 * B.delta; // cells claim the primitives whose (already inflated) boxes come this close; the device grows a ray's cell rectangle by its own position error
            const double csx = ex / G, csz = ez / G;
            std::vector<std::vector<int>> cell_items((size_t)G * G);
            for (size_t i = 0; i < layer.size(); ++i) {
                int cr[4];
                grid_cell_range(layer[i].b, lb, G, csx, csz, eps, cr);
                const int i0 = cr[0], i1 = cr[1], j0 = cr[2], j1 = cr[3];
                if (rec) std::memcpy(&rec->cell[(size_t)layer[i].idx * 4], cr, sizeof cr);
                for (int j = j0; j <= j1; ++j) for (int ii = i0; ii <= i1; ++ii) cell_items[(size_t)j * G + ii].push_back((int)i);
            }
            size_t claimed = 0;
            for (const std::vector<int> &ci : cell_items) claimed += ci.size();
            if (claimed > 4 * layer.size()) cell_items.clear(); // primitives that each span many cells (long sweeps, slabs): the per-cell trees would multiply them -- no grid
            const int depth0 = 3; // stack entries a grid start may already hold: the rectangle's tree under the tall tree (+ margin)
            auto subtree = [&](const std::vector<BvhItem> &its) -> int { // child code of a tree over `its`, appended to B.nodes
                if (its.empty()) return RTMI_BVH_EMPTY;
                const int b0 = (int)B.items.size();
                B.items.insert(B.items.end(), its.begin(), its.end());
                if (its.size() == 1) return B.lone(its[0]);
                return B.build(b0, b0 + (int)its.size(), depth0);
            };
            // One tree per RECTANGLE of cells a segment can touch -- 1 x 1, 2 x 1, 1 x 2, 2 x 2 (four families, each indexed by the rectangle's low corner:
            // grid_cells[(wi + 2 wj) G G + j0 G + i0]) -- over the union of the cells' primitives: a segment starts at ONE root (no root per cell to push and
            // to visit), and a primitive two cells of the rectangle share is in the tree once (it used to be tested exactly once per cell).
            if (!cell_items.empty()) grid_cells.assign((size_t)4 * G * G, RTMI_BVH_EMPTY);
            // The 4 G^2 rectangle trees (C3: 11 025 of them) are independent: every job builds its tree in a builder of its own, worker threads take jobs from a
            // shared counter, and the results are appended to the node array IN JOB ORDER with their node offsets rebased -- the same array whatever the thread
            // count (scene creation at C3: 59 ms single-threaded, most of it here).
            if (!cell_items.empty()) {
                struct RectTree { std::vector<float> nodes; int root = RTMI_BVH_EMPTY; int depth = 0; };
                const size_t n_jobs = (size_t)4 * G * G;
                std::vector<RectTree> trees(n_jobs);
                auto job = [&](size_t jb) {
                    const int fam = (int)(jb / ((size_t)G * G)), j = (int)((jb / (size_t)G) % (size_t)G), i = (int)(jb % (size_t)G);
                    const int wi = fam & 1, wj = fam >> 1;
                    if (j + wj >= G || i + wi >= G) return;
                    std::vector<int> uni;
                    for (int dj = 0; dj <= wj; ++dj) for (int di = 0; di <= wi; ++di) { const std::vector<int> &ci = cell_items[(size_t)(j + dj) * G + i + di]; uni.insert(uni.end(), ci.begin(), ci.end()); }
                    std::sort(uni.begin(), uni.end());
                    uni.erase(std::unique(uni.begin(), uni.end()), uni.end());
                    if (uni.empty()) return;
                    BvhBuilder L;
                    L.flags = &B; L.delta = B.delta; L.sah_depth = B.sah_depth; L.min_frac = B.min_frac; L.sweep_max = B.sweep_max; L.sah_levels = B.sah_levels;
                    for (int k : uni) L.items.push_back(layer[(size_t)k]);
                    RectTree &T = trees[jb];
                    if (L.items.size() == 1) { T.root = L.lone(L.items[0]); T.depth = depth0 + 1; }
                    else { T.root = L.build(0, (int)L.items.size(), depth0); T.depth = L.max_depth; }
                    T.nodes.swap(L.nodes);
                };
                const double tr0 = now_ms();
                { // the whole tree (if deferred) is one more job of the same team
                    const std::function<void()> first = whole_job;
                    whole_job = nullptr;
                    parallel_blocks(n_jobs, 16, [&](size_t b, size_t e) { for (size_t q = b; q < e; ++q) job(q); }, first ? &first : nullptr);
                }
                if (K.debug) fprintf(stderr, "[rtmi] build: %zu rectangle trees on %u threads %.2f ms\n", n_jobs, build_threads(), now_ms() - tr0);
                join_whole();
                // append in job order, node offsets rebased: every job's place in the array is the sum of the sizes before it, so the copies run on the team too
                std::vector<size_t> at(n_jobs + 1, B.nodes.size());
                for (size_t jb = 0; jb < n_jobs; ++jb) { at[jb + 1] = at[jb] + trees[jb].nodes.size(); B.max_depth = std::max(B.max_depth, trees[jb].depth); }
                B.nodes.resize(at[n_jobs]);
                parallel_blocks(n_jobs, 64, [&](size_t b, size_t e) {
                    for (size_t jb = b; jb < e; ++jb) {
                        RectTree &T = trees[jb];
                        if (T.root == RTMI_BVH_EMPTY) continue;
                        const int base = (int)(at[jb] / 16) * 64;
                        float *dst = &B.nodes[at[jb]];
                        std::memcpy(dst, T.nodes.data(), T.nodes.size() * sizeof(float));
                        for (size_t nd = 0; nd < T.nodes.size() / 16; ++nd) {
                            int c[2];
                            std::memcpy(c, dst + nd * 16 + 12, 8);
                            for (int k = 0; k < 2; ++k) if (c[k] >= 0) c[k] += base; // inner node: byte offset of its record (leaf codes and RTMI_BVH_EMPTY are negative)
                            std::memcpy(dst + nd * 16 + 12, c, 8);
                        }
                        grid_cells[jb] = T.root + base;
                    }
                });
            }
            join_whole();
            if (d.bvh_root < 0) cell_items.clear(); // (the whole tree did not fit the stack: every ray takes the flat scan, no grid either)
            if (!cell_items.empty()) d.grid_tall = subtree(tall);
            if (cell_items.empty() || B.max_depth >= RTMI_BVH_STACK - 1 || B.nodes.size() / 16 >= (1u << 25)) { // too deep for the stack: no grid (the whole tree above stays valid)
                grid_cells.clear(); d.grid_tall = RTMI_BVH_EMPTY;
            } else {
                d.grid_n = G; d.grid_nf = (float)G; d.grid_nnf = (float)(G * G); d.grid_gmax = (float)(G - 1);
                d.grid_kmax = K.grid_kmax;
                d.grid_walk = d.grid_kmax >= 4 && K.grid_walk; // (RTMI_GRID_WALK=0, tests: the same grid without the piecewise walk)
                d.grid_lo_x = (float)lb.lo[0]; d.grid_lo_z = (float)lb.lo[2];
                d.grid_inv_x = (float)(1.0 / csx); d.grid_inv_z = (float)(1.0 / csz);
                d.grid_off_x = -d.grid_lo_x * d.grid_inv_x; d.grid_off_z = -d.grid_lo_z * d.grid_inv_z; // (float products: the bits the device used to compute per ray)
                d.grid_cs_x = (float)csx; d.grid_cs_z = (float)csz;
                for (int k = 0; k < 3; ++k) { d.grid_box[k] = f_down(lb.lo[k] - B.delta - eps); d.grid_box[3 + k] = f_up(lb.hi[k] + B.delta + eps); }
                d.grid_eps = 0.0f;
                BvhBox tb = box_empty();
                for (const BvhItem &it : tall) box_grow(tb, it.b);
                if (rec) {
                    rec->grid = true; rec->lb = lb; rec->tb = tb; rec->G = G; rec->csx = csx; rec->csz = csz; rec->eps = eps;
                    for (const BvhItem &it : layer) rec->cls[(size_t)it.idx] |= TB_LAYER;
                    for (const BvhItem &it : tall) rec->cls[(size_t)it.idx] |= TB_TALL;
                }
                for (int k = 0; k < 3; ++k) { d.grid_tall_box[k] = tall.empty() ? 0.0f : f_down(tb.lo[k] - B.delta - eps); d.grid_tall_box[3 + k] = tall.empty() ? 0.0f : f_up(tb.hi[k] + B.delta + eps); }
                for (int k = 0; k < 3; ++k) { // what the device tests: {lo, hi} half pairs, rounded outward once more
                    d.grid_box_h[k] = (unsigned)half_outward(d.grid_box[k], false) | ((unsigned)half_outward(d.grid_box[3 + k], true) << 16);
                    d.grid_tall_box_h[k] = (unsigned)half_outward(d.grid_tall_box[k], false) | ((unsigned)half_outward(d.grid_tall_box[3 + k], true) << 16);
                }
            }
        }
    }
    join_whole();
    // ---- neighbourhood trees of the media (DevScene::mloc_*) ------------------------------------------------------------------------------------------------
    d.n_mloc = 0;
    // (measured on make-final: node visits per segment 10.2 -> 8.3, frame 17.43 vs 17.46 ms -- the segments it shortens finish early and wait for their wave's
    // long ones; off unless RTMI_MLOC=1)
    if (media_boxes && d.bvh_root >= 0 && K.mloc) {
        const size_t n_tree = B.items.size(); // (the grid is never built for a scene with media: the items are the whole tree's)
        std::vector<BvhItem> world(B.items.begin(), B.items.end());
        for (const BvhBox &mb : *media_boxes) {
            if (d.n_mloc >= 4) break;
            BvhBox R = mb; // the boundary's box, a hundredth larger per side
            for (int k = 0; k < 3; ++k) { const double pad = 0.01 * (mb.hi[k] - mb.lo[k]) + 4.0 * B.delta; R.lo[k] -= pad; R.hi[k] += pad; }
            std::vector<BvhItem> its;
            for (const BvhItem &it : world) { // every primitive with a surface point inside R: its box (the tree inflates it by delta once more) reaches into R
                bool hit = true;
                for (int k = 0; k < 3; ++k) hit = hit && it.b.hi[k] + 2.0 * B.delta >= R.lo[k] && it.b.lo[k] - 2.0 * B.delta <= R.hi[k];
                if (hit) its.push_back(it);
            }
            if (its.size() * 2 > n_tree) continue; // a medium that holds most of the scene (make-final's haze): nothing to gain
            int root = RTMI_BVH_EMPTY;
            if (its.size() == 1) root = B.lone(its[0]);
            else if (!its.empty()) {
                const int b0 = (int)B.items.size();
                B.items.insert(B.items.end(), its.begin(), its.end());
                root = B.build(b0, b0 + (int)its.size(), 1);
            }
            if (B.max_depth >= RTMI_BVH_STACK - 1 || B.nodes.size() / 16 >= (1u << 25)) break; // (cannot happen: a subset of a tree that fitted)
            d.mloc_root[d.n_mloc] = root;
            for (int k = 0; k < 3; ++k) { d.mloc_box[d.n_mloc][k] = f_up(R.lo[k]); d.mloc_box[d.n_mloc][3 + k] = f_down(R.hi[k]); }
            d.n_mloc++;
        }
    }
    d.bvh_node16 = 0;
    if (d.bvh_root != RTMI_BVH_EMPTY) { // 32-byte records (Node16) when rounding the planes to half costs little: 12 halves + 2 child codes
        auto half_val = [](uint16_t b) { // the half's value (integer decode: no software _Float16 conversion)
            const int e = (b >> 10) & 31, m = b & 1023;
            const double v = e == 0 ? std::ldexp((double)m, -24) : (e == 31 ? (m ? (double)NAN : (double)INFINITY) : std::ldexp((double)(1024 + m), e - 25));
            return (b >> 15) ? -v : v;
        };
        std::vector<float> out(B.nodes.size() / 2, 0.0f);
        double area32 = 0.0, area16 = 0.0;
        const size_t n_nodes = B.nodes.size() / 16;
        std::vector<double> part32((n_nodes + 2047) / 2048 + 1, 0.0), part16(part32.size(), 0.0); // per block, summed in block order: the same sums whatever the thread count
        parallel_blocks(n_nodes, 2048, [&](size_t nb, size_t ne) {
            double a32 = 0.0, a16 = 0.0;
            for (size_t n = nb; n < ne; ++n) {
                const float *q = &B.nodes[n * 16];
                uint16_t h[12];
                for (int side = 0; side < 2; ++side) {
                    const float lo[3] = {q[side * 4], q[side * 4 + 1], q[8 + side * 2]}, hi[3] = {q[side * 4 + 2], q[side * 4 + 3], q[8 + side * 2 + 1]};
                    double e32[3], e16[3];
                    for (int k = 0; k < 3; ++k) {
                        h[side * 6 + k * 2] = half_outward(lo[k], false); h[side * 6 + k * 2 + 1] = half_outward(hi[k], true);
                        e32[k] = (double)hi[k] - lo[k]; e16[k] = half_val(h[side * 6 + k * 2 + 1]) - half_val(h[side * 6 + k * 2]);
                    }
                    if (e32[0] >= 0 && std::isfinite(e32[0] + e32[1] + e32[2])) { // (the lone primitive's empty sibling is +inf / -inf)
                        a32 += e32[0] * e32[1] + e32[1] * e32[2] + e32[2] * e32[0];
                        a16 += std::isfinite(e16[0] + e16[1] + e16[2]) ? e16[0] * e16[1] + e16[1] * e16[2] + e16[2] * e16[0] : INFINITY;
                    }
                }
                int c[2];
                std::memcpy(c, &q[12], 8);
                for (int k = 0; k < 2; ++k) if (c[k] >= 0 && c[k] != RTMI_BVH_EMPTY) c[k] /= 2; // byte offsets of 32-byte records
                std::memcpy(reinterpret_cast<char *>(&out[n * 8]), h, 24);
                std::memcpy(reinterpret_cast<char *>(&out[n * 8]) + 24, c, 8);
            }
            part32[nb / 2048] = a32; part16[nb / 2048] = a16;
        });
        for (size_t k = 0; k < part32.size(); ++k) { area32 += part32[k]; area16 += part16[k]; }
        const bool use16 = K.node16 >= 0 ? K.node16 == 1 : (area16 <= 1.25 * area32); // RTMI_NODE16 overrides the choice (tests)
        if (use16) {
            d.bvh_node16 = 1;
            d.bvh_root = d.bvh_root >= 0 ? d.bvh_root / 2 : d.bvh_root;
            for (int &c : grid_cells) if (c >= 0) c /= 2;
            for (int k = 0; k < d.n_mloc; ++k) if (d.mloc_root[k] >= 0) d.mloc_root[k] /= 2;
            if (d.grid_tall >= 0) d.grid_tall /= 2;
            return out;
        }
    }
    return B.nodes;
}

// ---- scene tables -----------------------------------------------------------------------------------------------------
// The caller's arrays of rtmi_scene_create_ex (already checked: every index is in range, every kind supported).
struct SceneArrays {
    int n_prims; const int32_t *prim_kind; const double *prim_geom; const int32_t *prim_mat;
    int n_mats; const int32_t *mat_kind; const int32_t *mat_tex; const double *mat_param;
    int n_tex; const int32_t *tex_kind; const double *tex_param; const int32_t *tex_child;
    int cam_kind; const double *cam; const int32_t *prim_flip; const int32_t *prim_xform;
    int n_xforms; const int32_t *xform_kind; const double *xform_param;
};

// The material half of a scene: the eleven device tables that read the materials, the textures and their assignment to the primitives (each named after its
// DevScene field), and the three host facts that depend on them.  pack_materials builds it -- for pack_scene, and for rtmi_scene_set_materials*, which
// rewrites these tables where they lie: one packer, so an edited scene holds the bytes a fresh one would.  Everything else of a scene reads geometry only.
struct PackedMaterials {
    std::vector<double> mat_rec, mat_grad, mat_param, tex_param;
    std::vector<int> prim_kind, prim_km, prim_mat, mat_kind, mat_tex, tex_kind, tex_child;
    bool has_ext = false; // the materials' share of DevScene::has_ext: a section 8(f4) texture, or a primitive whose material is Isotropic
    bool uses_perlin = false;
    int max_image = -1;
    int defer_mat = -1; // DevScene::defer_mat: the scene's deferred emitter (pack_materials)
};

// What a scene uploads, as host tables (each named after its DevScene field), plus what rtmi_scene keeps on the host.
struct PackedScene {
    DevScene d{}; // scalar fields; the table pointers stay null until the upload
    std::vector<double> stat_geom, stat4_d, exact12, ext_xf, leaf_rec, mov_geom;
    std::vector<float> stat4_f, bvh_nodes, cull20;
    std::vector<int> stat_orig, grid_cells, moving_all, ext_info, mov_orig;
    PackedMaterials M;
    std::vector<int> host_kind; // primitive kinds, boundary flag removed
    std::map<int, std::array<double, 5>> media_fast_of;
    int bvh_node_count = 0, bvh_depth = 0;
    TreeBuild tree;        // what build_bvh was given and decided (rtmi_scene_set_geometry)
    bool geom_ext = false; // the geometry's share of DevScene::has_ext: a primitive the sphere kernels do not hold (d.has_ext = geom_ext || M.has_ext)
    double t_tree0 = 0.0, t_tree1 = 0.0; // now_ms() around the tree build (RTMI_DEBUG)
};

// Pads a table of `rec`-value records to round_up(n, 8) + 8 records with copies of the last (the scans read whole groups past the end).
template <typename T> void pad_last(std::vector<T> &v, size_t rec) {
    const size_t n = v.size() / rec;
    if (n == 0) return;
    const std::vector<T> last(v.end() - (long)rec, v.end());
    while (v.size() < ((n + 7) / 8 * 8 + 8) * rec) v.insert(v.end(), last.begin(), last.end());
}

// Which UV coordinates each texture reads -- bit 0: u, bit 1: v (texture.clj: UVGradient -- per coordinate: a gradient whose corner colours do not vary
// along u never reads u --, ImageMap, through Checkerboard / FlipTexture children); Constant, Checkerboard itself and the Perlin family read p only
std::vector<char> texture_uv_use(const SceneArrays &a) {
    std::vector<char> uses((size_t)std::max(a.n_tex, 1), 0);
    bool changed = true;
    for (int pass = 0; pass <= a.n_tex && changed; ++pass) { // children may come after their parents: iterate to the fixed point (a pass that changes nothing ends it:
        changed = false;                                    // one texture per sphere made the unconditional n_tex passes 5.8 of the 6.4 s a 90 000-sphere scene took to create)
        for (int t = 0; t < a.n_tex; ++t) {
            const int k = a.tex_kind[t];
            char u = k == RTMI_TEX_IMAGE ? 3 : 0;
            if (k == RTMI_TEX_UVGRADIENT) { // co cu cv cuv: a = cu (1-u) + co u, b = cuv (1-u) + cv u, out = b (1-v) + a v  (texture.clj:26-34)
                const double *tp = a.tex_param + (size_t)t * RTMI_TEX_STRIDE;
                bool var_u = false, var_v = false;
                // "does not vary" is a comparison of BITS (memcmp), not of values: only then is the lerp of the two colours at u = 1/2 the colour itself
                // whatever it holds (c/2 + c/2 = c exactly; +0 against -0, or two different NaNs, count as varying and keep the real coordinate)
                auto same = [&](int x, int y) { return std::memcmp(&tp[x], &tp[y], sizeof(double)) == 0; };
                for (int c = 0; c < 3; ++c) {
                    var_u = var_u || !same(c, 3 + c) || !same(6 + c, 9 + c); // co != cu or cv != cuv
                    var_v = var_v || !same(c, 6 + c) || !same(3 + c, 9 + c); // co != cv or cu != cuv
                }
                u = (char)((var_u ? 1 : 0) | (var_v ? 2 : 0));
            }
            if (k == RTMI_TEX_CHECKER || k == RTMI_TEX_FLIP_U || k == RTMI_TEX_FLIP_V)
                for (int c = 0; c < (k == RTMI_TEX_CHECKER ? 2 : 1); ++c) {
                    const int ch = a.tex_child[2 * (size_t)t + c];
                    if (ch >= 0 && ch < a.n_tex) u |= uses[(size_t)ch];
                }
            if (uses[(size_t)t] != u) { uses[(size_t)t] = u; changed = true; }
        }
    }
    return uses;
}

// DevScene::cam_fixed_origin of a camera (pack_scene, rtmi_scene_set_camera*): get-ray's origin is cam origin + lens offset; with aperture 0 the offset is
// (+-0, +-0, +-0) (camera.clj:39-44: lens-radius * rand-in-unit-disk), and x + (+-0) = x bit for bit for every x except -0 (whose sum with +0 is +0): then, and
// for the pinhole camera, all rays share one origin
// (a component may be neither -0 nor infinite in EITHER precision: the FP32 kernels read (float)cam[k], and a tiny negative double is -0.0f there)
inline bool camera_component_plain(double v) { return std::isfinite(v) && std::isfinite((float)v) && !(std::signbit(v) && (float)v == 0.0f); }
inline int camera_fixed_origin(int cam_kind, const double *cam) {
    bool fixed = cam_kind == RTMI_CAM_PINHOLE || cam[21] == 0.0;
    for (int k = 0; k < 3; ++k) fixed = fixed && camera_component_plain(cam[k]);
    for (int k = 12; k < 18; ++k) fixed = fixed && std::isfinite(cam[k]) && std::isfinite((float)cam[k]);
    return fixed ? 1 : 0;
}
// TraceParams::fixed_rays of a thin-lens camera with a fixed origin: the lens offset (+-0, +-0, +-0) is also subtracted from the direction (camera.clj:44-46), which
// it changes only where the direction before it is -0.  That is lleft + s horiz + t vert - origin, a left fold of sums: a sum is -0 only when both terms are,
// so a lower-left corner without a -0 component rules it out and the wave-wide refill may skip the disk's values and keep their draw count.
inline int camera_fixed_rays(int cam_kind, int fixed_origin, const double *cam) {
    bool fixed = cam_kind == RTMI_CAM_THINLENS && fixed_origin;
    for (int k = 3; k < 6; ++k) fixed = fixed && camera_component_plain(cam[k]);
    return fixed ? 1 : 0;
}
// The shutter interval of a camera: the times its rays carry (camera.clj:16: a pinhole ray has time 0; camera.clj:48: a thin lens draws t0 + (t1 - t0) * rand)
inline void camera_shutter(int cam_kind, const double *cam, double &t_lo, double &t_hi) {
    t_lo = cam_kind == RTMI_CAM_THINLENS ? std::min(cam[22], cam[23]) : 0.0;
    t_hi = cam_kind == RTMI_CAM_THINLENS ? std::max(cam[22], cam[23]) : 0.0;
}

// PackedScene::geom_ext from the arrays alone, for the host-only test hook rtmi_test_pack_materials, which has no built scene to ask (creation and the live edits
// pass the flag pack_geometry computed): a kind beyond the spheres, a medium's boundary, an instance wrapper, a flip.  prim_flip / prim_xform may be null (none)
inline bool geometry_is_ext(const SceneArrays &a) {
    for (int i = 0; i < a.n_prims; ++i) {
        const int kind = a.prim_kind[i] & ~RTMI_PRIM_BOUNDARY;
        if ((a.prim_kind[i] & RTMI_PRIM_BOUNDARY) || kind > RTMI_PRIM_MOVING || (a.prim_xform && a.prim_xform[2 * i + 1] != 0) || (a.prim_flip && a.prim_flip[i])) return true;
    }
    return false;
}

// The material half of pack_scene.  Of `a` it reads the primitive count, kinds and materials and the material and texture tables -- no geometry, no camera.
// geom_ext: PackedScene::geom_ext of the scene these materials belong to (a mixed-kind scene has no deferred emitter).
PackedMaterials pack_materials(const SceneArrays &a, bool geom_ext) {
    PackedMaterials M;
    const int n_prims = a.n_prims;
    for (int t = 0; t < a.n_tex; ++t) {
        if (a.tex_kind[t] > RTMI_TEX_CHECKER) M.has_ext = true; // section 8(f4) textures live in the EXT kernels only
        if (a.tex_kind[t] >= RTMI_TEX_PERLIN_NOISE && a.tex_kind[t] <= RTMI_TEX_MARBLE) M.uses_perlin = true;
        if (a.tex_kind[t] == RTMI_TEX_IMAGE) M.max_image = std::max(M.max_image, (int)a.tex_param[(size_t)t * RTMI_TEX_STRIDE]);
    }
    for (int i = 0; i < n_prims; ++i)
        if (a.mat_kind[a.prim_mat[i]] == RTMI_MAT_ISOTROPIC) M.has_ext = true; // Isotropic.scatter (shader.clj:129-138) is compiled into the EXT kernels only
    // device copy of prim_kind: + RTMI_PRIM_NEEDS_U / _V where a UVSphere's material texture reads that coordinate; + RTMI_PRIM_NEEDS_UV where a rectangle's or
    // a triangle's does (its uv is two IEEE divisions per hit (hitable.clj:283-284), a triangle's a second Moeller-Trumbore: computed only where the material's
    // texture reads uv at all -- both coordinates then: no coordinate is ever replaced here, so nothing deviates --; a Cornell box's walls never do)
    const std::vector<char> uses = texture_uv_use(a);
    M.prim_mat.assign(a.prim_mat, a.prim_mat + n_prims);
    M.prim_kind.resize((size_t)n_prims);
    for (int i = 0; i < n_prims; ++i) {
        const int kind = a.prim_kind[i] & ~RTMI_PRIM_BOUNDARY;
        M.prim_kind[(size_t)i] = kind;
        const int m = M.prim_mat[(size_t)i], t = (m >= 0 && m < a.n_mats) ? a.mat_tex[m] : -1;
        if (kind == RTMI_PRIM_UVSPHERE) {
            const int bits = (t < 0 || t >= a.n_tex) ? 3 : uses[(size_t)t];
            if (bits & 1) M.prim_kind[(size_t)i] |= RTMI_PRIM_NEEDS_U;
            if (bits & 2) M.prim_kind[(size_t)i] |= RTMI_PRIM_NEEDS_V;
        } else if (kind >= RTMI_PRIM_RECT_XY && kind <= RTMI_PRIM_TRIANGLE) {
            if (t < 0 || t >= a.n_tex || uses[(size_t)t]) M.prim_kind[(size_t)i] |= RTMI_PRIM_NEEDS_UV;
        }
    }
    M.prim_km.assign((size_t)std::max(n_prims, 1) * 2, 0);
    for (int i = 0; i < n_prims; ++i) { M.prim_km[2 * (size_t)i] = M.prim_kind[(size_t)i]; M.prim_km[2 * (size_t)i + 1] = M.prim_mat[(size_t)i]; }
    // The deferred emitter of a sphere-only scene: the ONE material that is a DiffuseLight, whose texture is a UVGradient (evaluated from mat_grad) that reads v
    // and not u, and that sits on UVSpheres only (on one at least).  A path that ends on it -- the cover scene's sky: nearly every path -- needs nothing of the hit
    // but the normal's y, and nothing reads the result but the fold: a launch that defers stores {atten, ny} and the fold finishes the sample.  Its primitives carry
    // RTMI_PRIM_DEFERRED beside RTMI_PRIM_NEEDS_V in prim_km (every kernel but the deferring twins still computes v for them; prim_kind, which the mixed-kind
    // kernels read, keeps its bits).  Two candidates, or none: no deferred emitter, and not one byte of the tables differs from what they were.
    if (!M.has_ext && !geom_ext) {
        std::vector<char> on_uv((size_t)std::max(a.n_mats, 1), 0), on_other((size_t)std::max(a.n_mats, 1), 0);
        for (int i = 0; i < n_prims; ++i) {
            const int m = M.prim_mat[(size_t)i];
            if (m < 0 || m >= a.n_mats) continue;
            ((M.prim_kind[(size_t)i] & 15) == RTMI_PRIM_UVSPHERE ? on_uv : on_other)[(size_t)m] = 1;
        }
        int n_cand = 0, cand = -1;
        for (int m = 0; m < a.n_mats; ++m) {
            const int t = a.mat_tex[m];
            if (a.mat_kind[m] != RTMI_MAT_DIFFUSE_LIGHT || t < 0 || t >= a.n_tex || a.tex_kind[t] != RTMI_TEX_UVGRADIENT || uses[(size_t)t] != 2) continue;
            if (!on_uv[(size_t)m] || on_other[(size_t)m]) continue;
            ++n_cand; cand = m;
        }
        if (n_cand == 1) {
            M.defer_mat = cand;
            for (int i = 0; i < n_prims; ++i)
                if (M.prim_mat[(size_t)i] == cand) M.prim_km[2 * (size_t)i] |= RTMI_PRIM_DEFERRED;
        }
    }
    // MatRec (rtmi_device.h) of every material, and the four corner colours of those whose texture is a UVGradient
    M.mat_rec.assign((size_t)std::max(a.n_mats, 1) * 12, 0.0);
    M.mat_grad.assign((size_t)std::max(a.n_mats, 1) * 12, 0.0);
    for (int m = 0; m < a.n_mats; ++m) {
        MatRec r;
        std::memset(&r, 0, sizeof(r));
        r.mat_kind = a.mat_kind[m]; r.tex = a.mat_tex[m]; r.param = a.mat_param[m];
        if (a.mat_kind[m] == RTMI_MAT_DIELECTRIC) { // one IEEE operation each, as the kernel would evaluate them per scatter
            const volatile double ri = a.mat_param[m];
            const volatile double inv = 1.0 / ri, num = 1.0 - ri, den = 1.0 + ri;
            const volatile double q = num / den;
            const volatile double r0 = q * q;
            r.inv_ri = inv; r.r0 = r0;
        }
        r.tex_kind = (r.tex >= 0 && r.tex < a.n_tex) ? a.tex_kind[r.tex] : -1;
        if (r.tex_kind == RTMI_TEX_CONSTANT) { const double *tp = a.tex_param + (size_t)r.tex * RTMI_TEX_STRIDE; r.r = tp[0]; r.g = tp[1]; r.b = tp[2]; }
        if (r.tex_kind == RTMI_TEX_UVGRADIENT) { // texture.clj:26-34: co cu cv cuv travel with the material
            std::memcpy(&M.mat_grad[(size_t)m * 12], a.tex_param + (size_t)r.tex * RTMI_TEX_STRIDE, 12 * sizeof(double));
            r.tex_kind = RTMI_TEX_GRADIENT_REC;
        }
        if (r.tex_kind == RTMI_TEX_CHECKER) { // both children Constant: the whole texture fits the record
            const int c0 = a.tex_child[2 * (size_t)r.tex], c1 = a.tex_child[2 * (size_t)r.tex + 1];
            if (c0 >= 0 && c0 < a.n_tex && c1 >= 0 && c1 < a.n_tex && a.tex_kind[c0] == RTMI_TEX_CONSTANT && a.tex_kind[c1] == RTMI_TEX_CONSTANT) {
                const double *t0 = a.tex_param + (size_t)c0 * RTMI_TEX_STRIDE, *t1 = a.tex_param + (size_t)c1 * RTMI_TEX_STRIDE;
                r.tex_kind = RTMI_TEX_CHECKER2;
                r.scale = a.tex_param[(size_t)r.tex * RTMI_TEX_STRIDE];
                r.r = t0[0]; r.g = t0[1]; r.b = t0[2]; r.c1r = t1[0]; r.c1g = t1[1]; r.c1b = t1[2];
            }
        }
        static_assert(sizeof(MatRec) == 96, "MatRec is twelve doubles");
        std::memcpy(&M.mat_rec[(size_t)m * 12], &r, sizeof(r));
    }
    M.mat_kind.assign(a.mat_kind, a.mat_kind + a.n_mats); M.mat_tex.assign(a.mat_tex, a.mat_tex + a.n_mats); M.mat_param.assign(a.mat_param, a.mat_param + a.n_mats);
    M.tex_kind.assign(a.tex_kind, a.tex_kind + a.n_tex); M.tex_child.assign(a.tex_child, a.tex_child + 2 * (size_t)a.n_tex);
    M.tex_param.assign(a.tex_param, a.tex_param + (size_t)a.n_tex * RTMI_TEX_STRIDE);
    return M;
}

// What the geometry half of a scene hands to the tree build: every primitive's world box, and the Boxes found among the rectangles
struct GeomExtras {
    std::vector<BvhBox> wbox;
    std::vector<char> bounded, box_first;
    int n_world = 0, n_media = 0, media[16];
};
// The geometry half of pack_scene, trees excluded: stat_geom, stat4_d, stat4_f, exact12, cull20, leaf_rec, ext_xf, mov_geom and media_fast_of (with the index
// tables that go with them) and the per-primitive wbox / bounded.  Of `a` it reads the primitives' kinds, geometry, flips and instance chains -- no material, no
// camera: the shutter interval [t_lo, t_hi] the MovingSphere bounds hold for is an argument (creation: the camera's; rtmi_scene_set_geometry: the built one).
// Writes the geometry fields of P.d (n_static, n_moving, n_all, cull_t_*, n_media, media_idx, media_lo, n_moving_all) and nothing else of it.
void pack_geometry(const SceneArrays &a, bool box_leaf, double t_lo, double t_hi, PackedScene &P, GeomExtras &X) {
    DevScene &d = P.d;
    const int n_prims = a.n_prims;
    int &n_world = X.n_world, &n_media = X.n_media, *media = X.media;
    for (int k = 0; k < a.n_xforms; ++k) {
        const double *p = a.xform_param + (size_t)k * 3;
        const double rec[4] = {a.xform_kind[k] == RTMI_XFORM_TRANSLATE ? 0.0 : 1.0, p[0], p[1], p[2]};
        P.ext_xf.insert(P.ext_xf.end(), rec, rec + 4);
    }
    // One pass over the primitives.  ext_info[i] = kind, FlipNormals parity, first xform, xform count: the one reading of the primitive that the tables below share.
    // Spheres and MovingSpheres without wrappers also go to the sphere kernels' tables: stat4 = {cx, cy, cz, r*r} (hitable.clj:188 (* radius radius), one IEEE
    // multiply in the precision the kernel computes in).  exact12[i] = c0.xyz, r*r, c1.xyz, t0, t1, moving?, r, 0 and the FP32 cull entry of scan variant
    // SCAN_SGPR_CULL: a MovingSphere's bounds its sweep over the camera's shutter interval [t_lo, t_hi] (rays outside that interval bypass the cull, make_cull_ray):
    // centre = midpoint of the two extreme centres, radius = r + half the distance between them, both inflated for the float rounding of the centre.
    std::vector<float> cull; // per primitive: centre (3), r2, w
    std::vector<BvhBox> &wbox = X.wbox;
    std::vector<char> &bounded = X.bounded;
    wbox.assign((size_t)n_prims, BvhBox{});
    bounded.assign((size_t)n_prims, 0);
    std::vector<int> &pk = P.host_kind;
    pk.resize((size_t)n_prims);
    for (int i = 0; i < n_prims; ++i) {
        const double *g = a.prim_geom + (size_t)i * RTMI_PRIM_STRIDE;
        const int kind = a.prim_kind[i] & ~RTMI_PRIM_BOUNDARY;
        const bool is_boundary = (a.prim_kind[i] & RTMI_PRIM_BOUNDARY) != 0;
        const int xf_first = a.prim_xform ? a.prim_xform[2 * i] : 0, xf_count = a.prim_xform ? a.prim_xform[2 * i + 1] : 0;
        const int info[4] = {kind, a.prim_flip ? (a.prim_flip[i] & 1) : 0, xf_first, xf_count};
        P.ext_info.insert(P.ext_info.end(), info, info + 4);
        pk[(size_t)i] = kind;
        if (!is_boundary) n_world = i + 1;
        if (kind == RTMI_PRIM_MEDIUM) { // not a surface: no box, a neutral cull entry (ext_prim_test ignores it), evaluated by ext_medium_test
            media[n_media++] = i;
            P.geom_ext = true;
            P.exact12.insert(P.exact12.end(), {g[0], g[1], g[2], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0});
            cull.insert(cull.end(), {0.0f, 0.0f, 0.0f, 0.0f, 0.0f});
            continue;
        }
        const bool sphere_kernels = !is_boundary && kind <= RTMI_PRIM_MOVING && xf_count == 0 && !(a.prim_flip && a.prim_flip[i]);
        if (!sphere_kernels) P.geom_ext = true;
        bounded[(size_t)i] = prim_world_box(kind, g, a.xform_kind, a.xform_param, xf_first, xf_count, t_lo, t_hi, wbox[(size_t)i]);
        const bool moving = kind == RTMI_PRIM_MOVING;
        const volatile double r2d = g[3] * g[3];
        if (sphere_kernels && moving) {
            P.mov_geom.insert(P.mov_geom.end(), g, g + RTMI_PRIM_STRIDE);
            P.mov_orig.push_back(i);
        } else if (sphere_kernels) {
            P.stat_geom.insert(P.stat_geom.end(), g, g + 4);
            P.stat_orig.push_back(i);
            const volatile float rf = (float)g[3];
            const volatile float r2f = rf * rf;
            P.stat4_d.insert(P.stat4_d.end(), {g[0], g[1], g[2], (double)r2d});
            P.stat4_f.insert(P.stat4_f.end(), {(float)g[0], (float)g[1], (float)g[2], (float)r2f});
        }
        if (kind > RTMI_PRIM_MOVING) P.exact12.insert(P.exact12.end(), {g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], 0.0, 0.0, 0.0});
        else P.exact12.insert(P.exact12.end(), {g[0], g[1], g[2], (double)r2d, g[4], g[5], g[6], g[7], g[8], moving ? 1.0 : 0.0, g[3], 0.0});
        if (kind > RTMI_PRIM_MOVING || xf_count > 0) { // f3 primitive or instanced sphere: cull by the sphere around its world box
            float cf[3] = {0, 0, 0};
            double r2b = 3.0e38, w = 3.0e38;
            if (bounded[(size_t)i]) {
                const BvhBox &b = wbox[(size_t)i];
                double slack = 0.0, rb2 = 0.0, cn = 0.0;
                for (int k = 0; k < 3; ++k) {
                    const double cm = 0.5 * (b.lo[k] + b.hi[k]);
                    cf[k] = (float)cm;
                    slack += std::fabs(cm - (double)cf[k]);
                    rb2 += 0.25 * (b.hi[k] - b.lo[k]) * (b.hi[k] - b.lo[k]);
                    cn += std::fabs((double)cf[k]);
                }
                const double rb = (std::sqrt(rb2) + slack + 1e-4) * (1.0 + 1e-6); // 1e-4: the reference's own rect/triangle bbox padding scale
                r2b = rb * rb * (1.0 + 1e-6);
                w = (2.0 * (cn + slack) * (cn + slack) + r2b) * 1.0001;
                if (!std::isfinite(w) || w > 1e37) { w = 3.0e38; r2b = 3.0e38; }
            }
            cull.insert(cull.end(), {cf[0], cf[1], cf[2], (float)std::min(r2b * (1.0 + 1e-6), 3.0e38), (float)std::min(w, 3.0e38)});
            continue;
        }
        double cm[3] = {g[0], g[1], g[2]}, rb = std::fabs(g[3]);
        bool unbounded = false;
        if (moving) {
            const double f0 = (t_lo - g[7]) / (g[8] - g[7]), f1 = (t_hi - g[7]) / (g[8] - g[7]);
            if (!std::isfinite(f0) || !std::isfinite(f1)) unbounded = true;
            else {
                double half2 = 0.0;
                for (int k = 0; k < 3; ++k) {
                    const double a0 = g[k] * (1.0 - f0) + g[4 + k] * f0, a1 = g[k] * (1.0 - f1) + g[4 + k] * f1;
                    cm[k] = 0.5 * (a0 + a1);
                    half2 += 0.25 * (a1 - a0) * (a1 - a0);
                }
                rb += std::sqrt(half2) * (1.0 + 1e-9);
            }
        }
        float cf[3];
        double slack = 0.0;
        for (int k = 0; k < 3; ++k) { cf[k] = (float)cm[k]; slack += std::fabs(cm[k] - (double)cf[k]); }
        if (moving) rb = (rb + slack) * (1.0 + 1e-6); // the bounding sphere is defined around the FLOAT centre
        const double r2b = moving ? rb * rb * (1.0 + 1e-6) : (double)r2d;
        const double cn = std::fabs((double)cf[0]) + std::fabs((double)cf[1]) + std::fabs((double)cf[2]) + slack;
        double w = (2.0 * cn * cn + r2b) * 1.0001;
        if (unbounded || !std::isfinite(w) || w > 1e37) w = 3.0e38; // tol = inf: always passes to the exact test
        cull.insert(cull.end(), {cf[0], cf[1], cf[2], unbounded ? 3.0e38f : (float)std::min(r2b * (moving ? 1.0 + 1e-6 : 1.0), 3.0e38), (float)w});
    }
    d.n_static = (int)P.stat_orig.size(); d.n_moving = (int)P.mov_orig.size();
    pad_last(P.stat4_d, 4); // (see scan_static_pipe)
    pad_last(P.stat4_f, 4);
    // Box = six consecutive rectangles RectXY z1, RectXY z0, RectXZ y1, RectXZ y0, RectYZ x1, RectYZ x0 over one (x0 y0 z0) - (x1 y1 z1) and one instance
    // chain (hitable.clj:500-511, spliced in by the flattener): the tree gets one leaf for the six (ext_box_test); z0 goes to slot 5 of the first record
    std::vector<char> &box_first = X.box_first;
    box_first.assign((size_t)std::max(n_prims, 1), 0);
    if (box_leaf) // (measured: make-final 22.1 ms with box leaves against 21.2 without -- six face tests per leaf cost more than the 1.8 node visits they save; kept for experiments)
    for (int i = 0; i + 5 < n_world; ++i) {
        static const int want[6] = {RTMI_PRIM_RECT_XY, RTMI_PRIM_RECT_XY, RTMI_PRIM_RECT_XZ, RTMI_PRIM_RECT_XZ, RTMI_PRIM_RECT_YZ, RTMI_PRIM_RECT_YZ};
        bool ok = true;
        for (int k = 0; k < 6 && ok; ++k) {
            ok = pk[(size_t)i + k] == want[k];
            if (a.prim_xform) ok = ok && a.prim_xform[2 * (i + k)] == a.prim_xform[2 * i] && a.prim_xform[2 * (i + k) + 1] == a.prim_xform[2 * i + 1];
        }
        if (!ok) continue;
        const double *q = a.prim_geom + (size_t)i * RTMI_PRIM_STRIDE;
        const double x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3], z1 = q[4], z0 = q[RTMI_PRIM_STRIDE + 4];
        const double expect[6][5] = {{x0, y0, x1, y1, z1}, {x0, y0, x1, y1, z0}, {x0, z0, x1, z1, y1}, {x0, z0, x1, z1, y0}, {y0, z0, y1, z1, x1}, {y0, z0, y1, z1, x0}};
        for (int k = 0; k < 6 && ok; ++k) for (int c = 0; c < 5; ++c) ok = ok && std::memcmp(&q[(size_t)k * RTMI_PRIM_STRIDE + c], &expect[k][c], sizeof(double)) == 0; // bit for bit
        if (!ok) continue;
        box_first[(size_t)i] = 1;
        P.exact12[(size_t)i * 12 + 5] = z0;
        i += 5;
    }
    pad_last(P.exact12, 12);
    pad_last(cull, 5);
    P.cull20.resize(cull.size() / 20 * 20);
    for (size_t g = 0; g < P.cull20.size(); g += 20) // per group of 4 (padded) primitives: cx[4] cy[4] cz[4] r2[4] w[4]
        for (int k = 0; k < 4; ++k) for (int f = 0; f < 5; ++f) P.cull20[g + 4 * f + k] = cull[g + 5 * k + f];
    d.n_all = n_world; d.cull_t_lo = t_lo; d.cull_t_hi = t_hi; // the scans walk the world; boundary primitives are reached only through their medium
    d.n_media = n_media;
    for (int k = 0; k < n_media; ++k) { d.media_idx[k] = media[k]; d.media_lo[k] = media[k]; }
    for (int i = 0; i < n_world; ++i) if (pk[(size_t)i] == RTMI_PRIM_MOVING) P.moving_all.push_back(i);
    d.n_moving_all = (int)P.moving_all.size();
    // LeafRec (rtmi_device.h: ext_leaf_test): one 112-byte record per world primitive
    P.leaf_rec.assign((size_t)std::max(n_prims, 1) * RTMI_LEAF_REC_DOUBLES, 0.0);
    for (int i = 0; i < n_prims; ++i) {
        double *q = &P.leaf_rec[(size_t)i * RTMI_LEAF_REC_DOUBLES];
        const int *info = &P.ext_info[(size_t)i * 4];
        const int kind = info[0], xf_first = info[2], xf_count = info[3];
        int hdr[4] = {kind | (info[1] ? 0x100 : 0), 0, 0, 0}; // bit 8: FlipNormals parity (resolve_hit_ext)
        const bool simple = (kind == RTMI_PRIM_SPHERE || kind == RTMI_PRIM_UVSPHERE || (kind >= RTMI_PRIM_RECT_XY && kind <= RTMI_PRIM_RECT_YZ)) && xf_count <= 2;
        if (!simple) hdr[1] = 1; // generic: ext_prim_test
        else {
            for (int c = 0; c < 5; ++c) q[2 + c] = P.exact12[(size_t)i * 12 + c]; // sphere: c r*r (slot 4 unused) | rectangle: u0 v0 u1 v1 k
            for (int k = 0; k < xf_count; ++k) {
                const double *xp = a.xform_param + (size_t)(xf_first + k) * 3;
                hdr[2 + k] = a.xform_kind[xf_first + k] == RTMI_XFORM_TRANSLATE ? 1 : 2;
                q[7 + 3 * k] = xp[0]; q[8 + 3 * k] = xp[1]; q[9 + 3 * k] = xp[2];
            }
            if (box_first[(size_t)i]) q[13] = P.exact12[(size_t)i * 12 + 5]; // z0 of the Box whose first face this rectangle is
        }
        std::memcpy(q, hdr, sizeof hdr);
    }
    P.ext_info.insert(P.ext_info.end(), {RTMI_PRIM_MEDIUM, 0, 0, 0}); // one record past the end: scan_small_ext requests primitive i + 1's records while it tests primitive i
    for (int k = 0; k < n_media; ++k) { // media whose boundary is one plain sphere, neither under wrappers: their operands go into the descriptor (media_fast)
        const int m = media[k];
        const int fb = (int)a.prim_geom[(size_t)m * RTMI_PRIM_STRIDE + 1], nb = (int)a.prim_geom[(size_t)m * RTMI_PRIM_STRIDE + 2];
        if (nb != 1 || fb < 0 || fb >= n_prims) continue;
        if (pk[(size_t)fb] != RTMI_PRIM_SPHERE && pk[(size_t)fb] != RTMI_PRIM_UVSPHERE) continue;
        if (a.prim_xform && (a.prim_xform[2 * m + 1] != 0 || a.prim_xform[2 * fb + 1] != 0)) continue;
        const double *e = &P.exact12[0];
        P.media_fast_of[m] = {e[(size_t)m * 12], e[(size_t)fb * 12], e[(size_t)fb * 12 + 1], e[(size_t)fb * 12 + 2], e[(size_t)fb * 12 + 3]};
    }
}

// The tree step of pack_scene: the device's trees over the world primitives of a packed geometry (P.bvh_nodes, P.grid_cells, the bvh_* / grid_* / mloc_* fields
// of P.d, P.tree).  has_ext: the scene takes the EXT kernels, which use no entry grid.
void build_trees(const SceneArrays &a, const BuildKnobs &K, bool has_ext, const GeomExtras &X, PackedScene &P) {
    DevScene &d = P.d;
    const double *cam = a.cam;
    const std::vector<BvhBox> &wbox = X.wbox;
    const std::vector<char> &bounded = X.bounded, &box_first = X.box_first;
    const std::vector<int> &pk = P.host_kind;
    const int n_world = X.n_world, n_media = X.n_media, *media = X.media;
    // ---- the trees ----
    P.t_tree0 = now_ms();
    std::vector<BvhBox> media_boxes; // per ConstantMedium: the box of its boundary (if every boundary primitive can be bounded)
    for (int k = 0; k < n_media; ++k) {
        const double *mg = a.prim_geom + (size_t)media[k] * RTMI_PRIM_STRIDE;
        const int fb = (int)mg[1], nb = (int)mg[2];
        BvhBox u = box_empty();
        bool ok = true;
        for (int q = fb; q < fb + nb; ++q) { ok = ok && bounded[(size_t)q]; if (ok) box_grow(u, wbox[(size_t)q]); }
        if (ok) media_boxes.push_back(u);
    }
    P.bvh_nodes = build_bvh(d, n_world, pk.data(), wbox, bounded, cam, !has_ext, P.grid_cells, box_first, K, &P.bvh_depth, &media_boxes, &P.tree);
    P.bvh_node_count = (int)(P.bvh_nodes.size() / (d.bvh_node16 ? 8 : 16));
    if (K.debug)
        fprintf(stderr, "[rtmi] tree: %d node records of %d bytes (%.2f MB), depth %d, %d big primitives, %d box leaves; entry grid %d x %d cells, %zu rectangle trees\n", P.bvh_node_count,
                d.bvh_node16 ? 32 : 64, P.bvh_node_count * (d.bvh_node16 ? 32.0 : 64.0) / 1e6, P.bvh_depth, d.n_big, (int)std::count(box_first.begin(), box_first.end(), (char)1), d.grid_n, d.grid_n, P.grid_cells.size());
    if (K.debug && d.n_mloc) fprintf(stderr, "[rtmi] %d medium neighbourhood tree(s)\n", d.n_mloc);
    P.t_tree1 = now_ms();
}

// The caller's (checked) arrays -> every device table of the scene, in host memory.  Pure host code: the same arrays and knobs give the same bytes.
PackedScene pack_scene(const SceneArrays &a, const BuildKnobs &K) {
    PackedScene P;
    DevScene &d = P.d;
    std::memset(&d, 0, sizeof d); // (padding included: the descriptor is uploaded as bytes)
    const double *cam = a.cam;
    d.n_tex = a.n_tex; d.cam_kind = a.cam_kind;
    std::memcpy(d.cam, cam, 24 * sizeof(double));
    d.cam_fixed_origin = camera_fixed_origin(a.cam_kind, cam);
    double t_lo, t_hi;
    camera_shutter(a.cam_kind, cam, t_lo, t_hi);
    GeomExtras X;
    pack_geometry(a, K.box_leaf, t_lo, t_hi, P, X);
    P.M = pack_materials(a, P.geom_ext); // (after the geometry: the deferred emitter wants a sphere-only scene)
    const int n_world = X.n_world;
    const bool has_ext = P.geom_ext || P.M.has_ext;
    build_trees(a, K, has_ext, X, P);
    d.has_ext = has_ext ? 1 : 0;
    d.defer_mat = has_ext ? -1 : P.M.defer_mat; // (pack_materials saw the same geometry: -1 already where has_ext)
    d.small_scan = (has_ext && n_world <= RTMI_SMALL_SCAN_MAX && K.small_scan) ? 1 : 0;
    return P;
}

} // namespace
