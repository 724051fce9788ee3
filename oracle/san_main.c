/* Stand-alone driver of the CPU oracle for its sanitized builds (make -C oracle sanitize; tests/test_host_sanitizers.py).
 * It reads a case file of the format tests/host_san/driver.cpp documents -- records { u32 name length, name, u32 type (0 u8, 1 i32, 2 i64, 3 u64, 4 f64),
 * u64 count, elements }, a record "call" = "<kind> <label>" starting each call -- runs the entry points oracle/oracle.py calls on the scene the call's
 * arrays describe, and prints one line per call with FNV-1a hashes of every output.  The test compares the lines with the hashes of what the ordinary
 * librt_oracle.so returns through oracle.py.  The oracle is compiled into this translation unit, so the scene struct is its own. */
#include "rt_oracle.c"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#define MAX_ARGS 48
typedef struct { char name[32]; uint32_t type; uint64_t count; unsigned char *bytes; } arg_t;
typedef struct { char kind[32], label[160]; int n_args; arg_t args[MAX_ARGS]; } call_t;

static const size_t ELEM[5] = {1, 4, 8, 8, 8};

static void die(const char *what) { fprintf(stderr, "san_main: %s\n", what); exit(2); }

static const arg_t *find(const call_t *c, const char *name) {
    for (int k = 0; k < c->n_args; ++k) if (strcmp(c->args[k].name, name) == 0) return &c->args[k];
    return NULL;
}
static const void *arr(const call_t *c, const char *name, uint32_t type) {
    const arg_t *a = find(c, name);
    if (!a) return NULL;
    if (a->type != type) die("an argument has another element type than the call reads");
    return a->bytes;
}
static int64_t scalar(const call_t *c, const char *name, int64_t otherwise) {
    const arg_t *a = find(c, name);
    if (!a) return otherwise;
    if (a->count != 1 || (a->type != 1 && a->type != 2 && a->type != 3)) die("a scalar argument is an array of one integer");
    return a->type == 1 ? *(const int32_t *)a->bytes : *(const int64_t *)a->bytes;
}
static double real_scalar(const call_t *c, const char *name, double otherwise) {
    const double *p = (const double *)arr(c, name, 4);
    return p ? p[0] : otherwise;
}
static uint64_t fnv1a(const void *p, size_t bytes) {
    uint64_t h = 1469598103934665603ull;
    const unsigned char *q = (const unsigned char *)p;
    for (size_t k = 0; k < bytes; ++k) { h ^= q[k]; h *= 1099511628211ull; }
    return h;
}
/* `bytes` zeroed bytes at exactly that size (the oracle's callers hand it zeroed arrays) */
static void *out_buf(size_t bytes) {
    void *p = calloc(bytes ? bytes : 1, 1);
    if (!p) die("out of memory");
    return p;
}

static rto_scene scene_of(const call_t *c) {
    rto_scene s;
    memset(&s, 0, sizeof s);
    s.n_prims = (int32_t)scalar(c, "n_prims", 0); s.n_mats = (int32_t)scalar(c, "n_mats", 0); s.n_tex = (int32_t)scalar(c, "n_tex", 0);
    s.prim_kind = arr(c, "prim_kind", 1); s.prim_geom = arr(c, "prim_geom", 4); s.prim_mat = arr(c, "prim_mat", 1);
    s.mat_kind = arr(c, "mat_kind", 1); s.mat_tex = arr(c, "mat_tex", 1); s.mat_param = arr(c, "mat_param", 4);
    s.tex_kind = arr(c, "tex_kind", 1); s.tex_param = arr(c, "tex_param", 4); s.tex_child = arr(c, "tex_child", 1);
    s.cam_kind = (int32_t)scalar(c, "cam_kind", 0); s.cam = arr(c, "cam", 4);
    s.n_nodes = (int32_t)scalar(c, "n_nodes", 0); s.root = (int32_t)scalar(c, "root", 0);
    s.node_kind = arr(c, "node_kind", 1); s.node_a = arr(c, "node_a", 1); s.node_d = arr(c, "node_d", 4);
    s.node_prim = arr(c, "node_prim", 1); s.node_children = arr(c, "node_children", 1);
    s.perlin_vec = arr(c, "perlin_vec", 4); s.perlin_perm = arr(c, "perlin_perm", 1);
    s.n_images = (int32_t)scalar(c, "n_images", 0);
    s.image_wh = arr(c, "image_wh", 1); s.image_off = arr(c, "image_off", 2); s.image_rgb = arr(c, "image_rgb", 0);
    return s;
}

static void run(const call_t *c) {
    const rto_scene s = scene_of(c);
    const int n = (int)scalar(c, "n", 0);
    printf("%s %s", c->label, c->kind);
    if (strcmp(c->kind, "render") == 0) {
        const int nx = (int)scalar(c, "nx", 0), ny = (int)scalar(c, "ny", 0);
        const size_t npix = (size_t)nx * (size_t)ny;
        double *lin = out_buf(npix * 3 * sizeof(double));
        uint8_t *q = out_buf(npix * 3);
        uint64_t cnt[2] = {0, 0};
        const int rc = rto_render(&s, nx, ny, (int)scalar(c, "ns", 0), (int)scalar(c, "depth", 50), (uint64_t)scalar(c, "seed", 0), 0, 0, nx, ny, lin, q, cnt,
                                  (int)scalar(c, "nthreads", 1));
        printf(" rc=%d linear=%016" PRIx64 " rgb8=%016" PRIx64 " counters=%" PRIu64 ",%" PRIu64, rc, fnv1a(lin, npix * 24), fnv1a(q, npix * 3), cnt[0], cnt[1]);
        free(lin); free(q);
    } else if (strcmp(c->kind, "probe_hit") == 0) {
        double *out = out_buf((size_t)n * 11 * sizeof(double));
        if (find(c, "bvh_seed")) rto_probe_hit_bvh(&s, (uint64_t)scalar(c, "bvh_seed", 0), n, arr(c, "rays", 4), real_scalar(c, "tmin", 0.001), real_scalar(c, "tmax", 0.0), out);
        else rto_probe_hit(&s, n, arr(c, "rays", 4), real_scalar(c, "tmin", 0.001), real_scalar(c, "tmax", 0.0), out);
        printf(" hits=%016" PRIx64, fnv1a(out, (size_t)n * 88));
        free(out);
    } else if (strcmp(c->kind, "probe_paths") == 0) {
        const int max_seg = (int)scalar(c, "max_seg", 0);
        double *rgb = out_buf((size_t)n * 24), *log = max_seg ? out_buf((size_t)n * max_seg * SEG_REC * sizeof(double)) : NULL;
        uint64_t *nseg = out_buf((size_t)n * 8);
        int32_t *nlog = out_buf((size_t)n * 4);
        rto_probe_paths(&s, n, arr(c, "rays", 4), arr(c, "keys", 3), (uint64_t)scalar(c, "ctr0", 0), (int)scalar(c, "depth", 50), rgb, nseg, log, max_seg, nlog);
        printf(" rgb=%016" PRIx64 " nseg=%016" PRIx64 " nlog=%016" PRIx64, fnv1a(rgb, (size_t)n * 24), fnv1a(nseg, (size_t)n * 8), fnv1a(nlog, (size_t)n * 4));
        if (log) printf(" log=%016" PRIx64, fnv1a(log, (size_t)n * max_seg * SEG_REC * sizeof(double)));
        free(rgb); free(log); free(nseg); free(nlog);
    } else if (strcmp(c->kind, "probe_camera") == 0) {
        double *out = out_buf((size_t)n * 64);
        rto_probe_camera(&s, n, arr(c, "uv", 4), arr(c, "keys", 3), out);
        printf(" rays=%016" PRIx64, fnv1a(out, (size_t)n * 64));
        free(out);
    } else if (strcmp(c->kind, "probe_texture") == 0) {
        double *out = out_buf((size_t)n * 24);
        rto_probe_texture(&s, (int)scalar(c, "tex", 0), n, arr(c, "uvp", 4), out);
        printf(" rgb=%016" PRIx64, fnv1a(out, (size_t)n * 24));
        free(out);
    } else if (strcmp(c->kind, "probe_scatter") == 0) {
        double *out = out_buf((size_t)n * 72);
        rto_probe_scatter(&s, (int)scalar(c, "mat", 0), n, arr(c, "rays", 4), arr(c, "hits", 4), arr(c, "keys", 3), out);
        printf(" out=%016" PRIx64, fnv1a(out, (size_t)n * 72));
        free(out);
    } else {
        die("unknown call kind");
    }
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc != 2) die("usage: san_main FILE");
    FILE *f = fopen(argv[1], "rb");
    if (!f) die("cannot open the case file");
    call_t *c = calloc(1, sizeof *c);
    int have = 0;
    for (;;) {
        uint32_t len, type;
        uint64_t count;
        char name[64];
        const int more = fread(&len, 4, 1, f) == 1;
        if (more) {
            if (len >= sizeof name || fread(name, 1, len, f) != len || fread(&type, 4, 1, f) != 1 || fread(&count, 8, 1, f) != 1 || type > 4 || count > (1ull << 31))
                die("bad record");
            name[len] = 0;
        }
        if (!more || strcmp(name, "call") == 0) { /* the call before this record is complete */
            if (have) run(c);
            for (int k = 0; k < c->n_args; ++k) free(c->args[k].bytes);
            memset(c, 0, sizeof *c);
            if (!more) break;
        }
        const size_t bytes = (size_t)count * ELEM[type];
        unsigned char *data = malloc(bytes ? bytes : 1); /* exactly the array: a read past an input is a report too */
        if (!data || (bytes && fread(data, 1, bytes, f) != bytes)) die("truncated record");
        if (strcmp(name, "call") == 0) {
            const char *sp = memchr(data, ' ', bytes);
            if (!sp || (size_t)(sp - (char *)data) >= sizeof c->kind || bytes - (size_t)(sp + 1 - (char *)data) >= sizeof c->label) die("bad call record");
            memcpy(c->kind, data, (size_t)(sp - (char *)data));
            memcpy(c->label, sp + 1, bytes - (size_t)(sp + 1 - (char *)data));
            free(data);
            have = 1;
        } else {
            if (!have || c->n_args == MAX_ARGS || len >= sizeof c->args[0].name) die("an array outside a call, too many arrays or too long a name");
            arg_t *a = &c->args[c->n_args++];
            memcpy(a->name, name, len + 1);
            a->type = type; a->count = count; a->bytes = data;
        }
    }
    free(c);
    fclose(f);
    return 0;
}
