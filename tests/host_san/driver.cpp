// Stand-alone driver of the library's host-only test hooks, for the sanitized builds (make -C raytrace_clj_amd/csrc sanitize; tests/test_host_sanitizers.py).
// It reads one case file (tests/san_cases.py writes it), calls the hooks of include/rtmi.h that are documented as host code only, and prints one line per
// call: the case's label, the call, the return code, every output and, last, the error text of a refused call.  The test compares each line with the
// line it computes from the ordinary librtmi.so.
// It never calls rtmi_init, a scene, render, probe or query entry, or a HIP function: a sanitized process opens no device.
//
// Case file: a flat sequence of records { u32 name length, name, u32 type (0 u8, 1 i32, 2 i64, 3 u64, 4 f64), u64 count, count elements, little endian }.
// A record named "call" (u8: "<kind> <label>") starts a call; the records up to the next "call" are its arguments by name.  An array that is missing is
// passed as NULL, a scalar is an array of one.  Every output buffer is allocated at exactly the size the call is told it has, filled with a pattern,
// and printed (or hashed) whole whatever the return code: a call that fails must leave the pattern, and one that writes past the end meets ASan.
//
//   driver FILE                      every call in file order, on the main thread
//   driver FILE --threads T ROUNDS   T threads start together behind a barrier; thread t runs call t % n_calls ROUNDS times; lines in thread order
//   driver --control heap|ub|race    one deliberate defect in THIS file (a read one past a new[], a signed overflow, an unsynchronised counter): the
//                                    sanitizers, their options and -fno-sanitize-recover must turn each into a report and a non-zero exit
#include "rtmi.h"

#include <cinttypes>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace {

struct Array {
    uint32_t type = 0;
    uint64_t count = 0;
    std::unique_ptr<unsigned char[]> bytes; // exactly count elements: a read past an input array is a report too
};
struct Call {
    std::string kind, label;
    std::map<std::string, Array> args;
};

const size_t kElem[5] = {1, 4, 8, 8, 8};
const unsigned char kFill = 0xA5;

[[noreturn]] void die(const char *what) {
    std::fprintf(stderr, "driver: %s\n", what);
    std::exit(2);
}

std::vector<Call> read_cases(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) die("cannot open the case file");
    std::vector<Call> calls;
    for (;;) {
        uint32_t len;
        if (std::fread(&len, 4, 1, f) != 1) break;
        if (len > 256) die("bad record name");
        std::string name(len, '\0');
        Array a;
        if (len && std::fread(&name[0], 1, len, f) != len) die("truncated record");
        if (std::fread(&a.type, 4, 1, f) != 1 || std::fread(&a.count, 8, 1, f) != 1 || a.type > 4 || a.count > (1ull << 31)) die("bad record header");
        const size_t bytes = (size_t)a.count * kElem[a.type];
        a.bytes.reset(new unsigned char[bytes ? bytes : 1]);
        if (bytes && std::fread(a.bytes.get(), 1, bytes, f) != bytes) die("truncated record");
        if (name == "call") {
            const std::string s((const char *)a.bytes.get(), bytes);
            const size_t sp = s.find(' ');
            if (sp == std::string::npos) die("a call record needs a kind and a label");
            calls.emplace_back();
            calls.back().kind = s.substr(0, sp);
            calls.back().label = s.substr(sp + 1);
        } else {
            if (calls.empty()) die("an array before the first call");
            calls.back().args[name] = std::move(a);
        }
    }
    std::fclose(f);
    return calls;
}

// ---- arguments ------------------------------------------------------------------------------------------------------------------------------------
template <class T> const T *arr(const Call &c, const char *name, uint32_t type) {
    auto it = c.args.find(name);
    if (it == c.args.end()) return nullptr;
    if (it->second.type != type) die("an argument has another element type than the call reads");
    return reinterpret_cast<const T *>(it->second.bytes.get());
}
const int32_t *i32s(const Call &c, const char *n) { return arr<int32_t>(c, n, 1); }
const uint64_t *u64s(const Call &c, const char *n) { return arr<uint64_t>(c, n, 3); }
const double *f64s(const Call &c, const char *n) { return arr<double>(c, n, 4); }
uint64_t count_of(const Call &c, const char *name) {
    auto it = c.args.find(name);
    return it == c.args.end() ? 0 : it->second.count;
}
int64_t scalar(const Call &c, const char *name, int64_t otherwise = 0) {
    auto it = c.args.find(name);
    if (it == c.args.end()) return otherwise;
    if (it->second.count != 1) die("a scalar argument is an array of one");
    if (it->second.type == 1) return *reinterpret_cast<const int32_t *>(it->second.bytes.get());
    if (it->second.type == 2) return *reinterpret_cast<const int64_t *>(it->second.bytes.get());
    die("a scalar argument is i32 or i64");
}

// ---- outputs ---------------------------------------------------------------------------------------------------------------------------------------
// `bytes` bytes of the pattern on the heap, at exactly that size (none: NULL)
std::unique_ptr<unsigned char[]> out_buf(int64_t bytes) {
    if (bytes <= 0) return nullptr;
    std::unique_ptr<unsigned char[]> p(new unsigned char[(size_t)bytes]);
    std::memset(p.get(), kFill, (size_t)bytes);
    return p;
}
uint64_t fnv1a(const void *p, int64_t bytes) {
    uint64_t h = 1469598103934665603ull;
    const unsigned char *q = static_cast<const unsigned char *>(p);
    for (int64_t k = 0; k < bytes; ++k) { h ^= q[k]; h *= 1099511628211ull; }
    return h;
}
struct Line {
    std::string s, err; // err: the text of a refused call, printed LAST on the line (it may hold anything, spaces and '=' included)
    Line(const Call &c) { s = c.label + " " + c.kind; }
    void num(const char *key, long long v) { char b[64]; std::snprintf(b, sizeof b, " %s=%lld", key, v); s += b; }
    void hex(const char *key, uint64_t v) { char b[64]; std::snprintf(b, sizeof b, " %s=%016" PRIx64, key, v); s += b; }
    template <class T> void list(const char *key, const T *v, int64_t n, bool as_hex = false) {
        s += std::string(" ") + key + "=";
        if (!v) { s += "null"; return; }
        s += "[";
        for (int64_t k = 0; k < n; ++k) {
            char b[40];
            if (as_hex) std::snprintf(b, sizeof b, "%s%" PRIx64, k ? "," : "", (uint64_t)v[k]);
            else std::snprintf(b, sizeof b, "%s%lld", k ? "," : "", (long long)v[k]);
            s += b;
        }
        s += "]";
    }
    void hash(const char *key, const void *p, int64_t bytes) { if (p) hex(key, fnv1a(p, bytes)); else s += std::string(" ") + key + "=null"; }
    void rc(int code) { num("rc", code); if (code != RTMI_OK) err = std::string(" err=") + rtmi_last_error(); }
    std::string str() const { return s + err; }
};

// creation's arrays, as rtmi_test_pack_materials / rtmi_test_pack_geometry take them
struct SceneArgs {
    int32_t n_prims, n_mats, n_tex, cam_kind, n_xforms;
    const int32_t *prim_kind, *prim_mat, *mat_kind, *mat_tex, *tex_kind, *tex_child, *prim_flip, *prim_xform, *xform_kind;
    const double *prim_geom, *mat_param, *tex_param, *cam, *xform_param;
    explicit SceneArgs(const Call &c)
        : n_prims((int32_t)scalar(c, "n_prims")), n_mats((int32_t)scalar(c, "n_mats")), n_tex((int32_t)scalar(c, "n_tex")), cam_kind((int32_t)scalar(c, "cam_kind")),
          n_xforms((int32_t)scalar(c, "n_xforms")), prim_kind(i32s(c, "prim_kind")), prim_mat(i32s(c, "prim_mat")), mat_kind(i32s(c, "mat_kind")),
          mat_tex(i32s(c, "mat_tex")), tex_kind(i32s(c, "tex_kind")), tex_child(i32s(c, "tex_child")), prim_flip(i32s(c, "prim_flip")),
          prim_xform(i32s(c, "prim_xform")), xform_kind(i32s(c, "xform_kind")), prim_geom(f64s(c, "prim_geom")), mat_param(f64s(c, "mat_param")),
          tex_param(f64s(c, "tex_param")), cam(f64s(c, "cam")), xform_param(f64s(c, "xform_param")) {}
};

// ---- the calls -------------------------------------------------------------------------------------------------------------------------------------
std::string run(const Call &c) {
    Line L(c);
    const std::string &k = c.kind;
    if (k == "build_tree") {
        auto hash = out_buf(8), info = out_buf(16), ms = out_buf(8);
        const int rc = rtmi_test_build_tree((int32_t)scalar(c, "n"), f64s(c, "geom"), f64s(c, "cam"), (int32_t)scalar(c, "threads"),
                                            scalar(c, "no_hash") ? nullptr : (uint64_t *)hash.get(), (int32_t *)info.get(), (double *)ms.get());
        L.rc(rc);
        L.hex("hash", *(uint64_t *)hash.get());
        L.list("info", (int32_t *)info.get(), 4);
    } else if (k == "pack_materials") {
        const SceneArgs a(c);
        auto hash = out_buf(8), facts = out_buf(12);
        const int rc = rtmi_test_pack_materials(a.n_prims, a.prim_kind, a.prim_geom, a.prim_mat, a.n_mats, a.mat_kind, a.mat_tex, a.mat_param, a.n_tex, a.tex_kind,
                                                a.tex_param, a.tex_child, a.cam_kind, a.cam, a.prim_flip, a.prim_xform, a.n_xforms, a.xform_kind, a.xform_param,
                                                (int32_t)scalar(c, "through_creation"), (uint64_t *)hash.get(), (int32_t *)facts.get());
        L.rc(rc);
        L.hex("hash", *(uint64_t *)hash.get());
        L.list("facts", (int32_t *)facts.get(), 3);
    } else if (k == "pack_geometry") {
        const SceneArgs a(c);
        auto hash = out_buf(8);
        const int rc = rtmi_test_pack_geometry(a.n_prims, a.prim_kind, a.prim_geom, a.prim_mat, a.n_mats, a.mat_kind, a.mat_tex, a.mat_param, a.n_tex, a.tex_kind,
                                               a.tex_param, a.tex_child, a.cam_kind, a.cam, a.prim_flip, a.prim_xform, a.n_xforms, a.xform_kind, a.xform_param,
                                               (int32_t)scalar(c, "through_creation"), (uint64_t *)hash.get());
        L.rc(rc);
        L.hex("hash", *(uint64_t *)hash.get());
    } else if (k == "refit") {
        // capacity: bytes of out_nodes (-1: NULL), cells_capacity: ints of out_cells (-1: NULL), leaf_floats: floats of out_leaf_box (0: NULL), want_big 0 / 1
        const int64_t cap = scalar(c, "capacity", -1), cells_cap = scalar(c, "cells_capacity", -1), leaf_floats = scalar(c, "leaf_floats"), want_big = scalar(c, "want_big");
        auto nodes = out_buf(cap), cells = out_buf(cells_cap > 0 ? cells_cap * 4 : 0), leaf = out_buf(leaf_floats * 4), big = out_buf(want_big ? 64 : 0);
        auto bytes = out_buf(8), info = out_buf(40);
        const int rc = rtmi_test_refit((int32_t)scalar(c, "n_prims"), i32s(c, "prim_kind"), i32s(c, "prim_flip"), i32s(c, "prim_xform"), (int32_t)scalar(c, "n_xforms"),
                                       i32s(c, "xform_kind"), (int32_t)scalar(c, "cam_kind"), f64s(c, "cam"), (int32_t)scalar(c, "n_steps"), f64s(c, "geoms"),
                                       f64s(c, "xforms"), nodes.get(), cap < 0 ? 0 : cap, (int64_t *)bytes.get(), (int32_t *)info.get(), (int32_t *)big.get(),
                                       (int32_t *)cells.get(), cells_cap < 0 ? 0 : cells_cap, leaf.get());
        L.rc(rc);
        L.num("bytes", *(int64_t *)bytes.get());
        L.list("info", (int32_t *)info.get(), 10);
        L.list("big", (int32_t *)big.get(), 16);
        L.hash("nodes", nodes.get(), cap);
        L.hash("cells", cells.get(), cells_cap * 4);
        L.hash("leaf_box", leaf.get(), leaf_floats * 4);
    } else if (k == "scene_lights") {
        const int64_t cap = scalar(c, "capacity"), alloc = scalar(c, "alloc", cap); // alloc: ints of out_prims (0: NULL); the capacity unless the case says otherwise
        auto prims = out_buf(alloc > 0 ? alloc * 4 : 0), count = out_buf(4);
        const int rc = rtmi_test_scene_lights((int32_t)scalar(c, "n_prims"), i32s(c, "prim_kind"), f64s(c, "prim_geom"), i32s(c, "prim_mat"), (int32_t)scalar(c, "n_mats"),
                                              i32s(c, "mat_kind"), i32s(c, "mat_tex"), (int32_t)scalar(c, "n_tex"), i32s(c, "tex_kind"), i32s(c, "prim_xform"),
                                              (int32_t)cap, (int32_t *)prims.get(), scalar(c, "no_count") ? nullptr : (int32_t *)count.get());
        L.rc(rc);
        L.num("count", *(int32_t *)count.get());
        L.list("prims", (int32_t *)prims.get(), alloc);
    } else if (k == "stage_layout") {
        const int64_t n = scalar(c, "n"), alloc = (int64_t)count_of(c, "elem_bytes");
        auto off = out_buf(alloc * 8), total = out_buf(8);
        const int rc = rtmi_test_stage_layout((int32_t)n, u64s(c, "elem_bytes"), u64s(c, "counts"), i32s(c, "present"), (uint64_t *)off.get(), (uint64_t *)total.get());
        L.rc(rc);
        L.hex("total", *(uint64_t *)total.get());
        L.list("offsets", (uint64_t *)off.get(), alloc, true);
    } else if (k == "halves") { // both roundings, both directions, of every x
        const double *x = f64s(c, "x");
        const int64_t n = (int64_t)count_of(c, "x");
        std::vector<int32_t> out((size_t)n * 4);
        for (int64_t i = 0; i < n; ++i)
            for (int up = 0; up < 2; ++up) {
                out[(size_t)i * 4 + up] = rtmi_test_half_outward(x[i], up);
                out[(size_t)i * 4 + 2 + up] = rtmi_test_refit_half(x[i], up);
            }
        L.list("half", out.data(), n * 4);
    } else if (k == "camera_fixed") {
        L.num("flags", rtmi_test_camera_fixed((int32_t)scalar(c, "cam_kind"), f64s(c, "cam")));
    } else if (k == "sample_keys") {
        const uint64_t *seed = u64s(c, "seed"), *pixel = u64s(c, "pixel"), *sample = u64s(c, "sample");
        const int64_t n = (int64_t)count_of(c, "seed");
        std::vector<uint64_t> out((size_t)n);
        for (int64_t i = 0; i < n; ++i) out[(size_t)i] = rtmi_sample_key(seed[i], pixel[i], sample[i]);
        L.list("keys", out.data(), n, true);
    } else if (k == "version") {
        L.num("version", rtmi_version());
    } else {
        die("unknown call kind");
    }
    return L.str();
}

// ---- the threads ------------------------------------------------------------------------------------------------------------------------------------
struct Barrier {
    std::mutex mu;
    std::condition_variable cv;
    int waiting = 0, need;
    explicit Barrier(int n) : need(n) {}
    void wait() {
        std::unique_lock<std::mutex> lk(mu);
        if (++waiting == need) cv.notify_all();
        else cv.wait(lk, [&] { return waiting == need; });
    }
};

int run_threads(const std::vector<Call> &calls, int n_threads, int rounds) {
    Barrier gate(n_threads);
    std::vector<std::vector<std::string>> lines((size_t)n_threads);
    std::vector<std::thread> team;
    for (int t = 0; t < n_threads; ++t)
        team.emplace_back([&, t] {
            const Call &c = calls[(size_t)t % calls.size()];
            gate.wait();
            for (int r = 0; r < rounds; ++r) lines[(size_t)t].push_back(run(c));
        });
    for (auto &th : team) th.join();
    for (int t = 0; t < n_threads; ++t)
        for (int r = 0; r < rounds; ++r) std::printf("t%d.r%d %s\n", t, r, lines[(size_t)t][(size_t)r].c_str());
    return 0;
}

// ---- the controls: defects of this file, on purpose ---------------------------------------------------------------------------------------------------
int g_plain_counter = 0;

int control(const std::string &what, int argc) {
    if (what == "heap") {
        volatile int *p = new int[4]{1, 2, 3, 4};
        const int v = p[3 + argc / 2]; // argc = 3: one past the end
        delete[] p;
        std::printf("control heap read %d\n", v);
    } else if (what == "ub") {
        volatile int big = 0x7fffffff;
        const int v = big + (argc - 2); // + 1
        std::printf("control ub computed %d\n", v);
    } else if (what == "race") {
        Barrier gate(2);
        auto bump = [&] { gate.wait(); for (int k = 0; k < 100000; ++k) g_plain_counter = g_plain_counter + 1; };
        std::thread a(bump), b(bump);
        a.join(); b.join();
        std::printf("control race counted %d\n", g_plain_counter);
    } else {
        die("--control heap|ub|race");
    }
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    if (argc == 3 && std::string(argv[1]) == "--control") return control(argv[2], argc);
    if (argc != 2 && !(argc == 5 && std::string(argv[2]) == "--threads")) die("usage: driver FILE [--threads T ROUNDS] | --control heap|ub|race");
    const std::vector<Call> calls = read_cases(argv[1]);
    if (calls.empty()) die("the case file holds no call");
    if (argc == 5) {
        const int t = std::atoi(argv[3]), r = std::atoi(argv[4]);
        if (t < 1 || t > 16 || r < 1) die("--threads T ROUNDS: 1 <= T <= 16, ROUNDS >= 1");
        return run_threads(calls, t, r);
    }
    for (const Call &c : calls) std::printf("%s\n", run(c).c_str());
    return 0;
}
