/*
 * rtmi.h -- C-ABI of librtmi.so: raytrace-clj's per-pixel Monte-Carlo sampling path on MI355X (gfx950).
 *
 * This is the drop-in boundary.  The reference (gonewest818/raytrace-clj) has no FFI of its own; the
 * seam this library replaces is the body of the render loop
 *     src/raytrace_clj/core.clj:100-108   (cp/upmap over tiled-coords -> pixel -> set-pixel)
 * i.e. everything `pixel` (core.clj:43-57) and `color` (core.clj:17-41) call through the Hitable /
 * Shader / Texture / Camera protocols (hitable.clj:7-10, shader.clj:22-24, texture.clj:8-9,
 * camera.clj:5-6).  A host (Clojure via JNA, Python via ctypes, C++) flattens a
 * {:camera c :world w} scene (scene.clj:321,331) into the arrays below and calls rtmi_render.
 * See INTEGRATION.md for the JNA stub.
 *
 * Conventions (normative):
 *   - plain C symbols, no exceptions cross the boundary;
 *   - every call returns int: 0 = RTMI_OK, < 0 = error class; rtmi_last_error() gives the text
 *     (thread-local, library-owned, valid until the next failing call on that thread);
 *   - rtmi_ctx / rtmi_scene are opaque, created and destroyed by the library only;
 *   - every host array argument is caller-allocated, caller-owned and only read/written for the
 *     duration of the call (the library keeps no host pointers);
 *   - host-side scalars and arrays are double / int32 whatever precision the kernels compute in;
 *   - a context is not re-entrant; distinct contexts may be driven from distinct threads;
 *   - framebuffers are row-major, RGB interleaved, ROW 0 = TOP, i.e. after the reference's flip
 *     y_out = ny-1-j (core.clj:105).
 *
 * Flat scene layout (what a flattener over the reference's records produces):
 *   primitives, in Hitlist order (hitable.clj:15-26):
 *     prim_kind[i]  RTMI_PRIM_SPHERE (hitable.clj:180) | RTMI_PRIM_UVSPHERE (:141) | RTMI_PRIM_MOVING (:224)
 *     prim_geom[i*9 + 0..8] = center0.xyz, radius, center1.xyz, t0, t1   (static: center1 = center0, t0 = 0, t1 = 1)
 *     prim_mat[i]   material index
 *   materials (shader.clj):
 *     mat_kind[m]   RTMI_MAT_LAMBERTIAN (:29) | RTMI_MAT_METAL (:46) | RTMI_MAT_DIELECTRIC (:76) | RTMI_MAT_DIFFUSE_LIGHT (:114)
 *     mat_tex[m]    texture index of albedo / emission (-1 for dielectric)
 *     mat_param[m]  fuzz (metal) | ri (dielectric) | 0
 *   textures (texture.clj):
 *     tex_kind[t]   RTMI_TEX_CONSTANT (:14) | RTMI_TEX_UVGRADIENT (:26) | RTMI_TEX_CHECKER (:44)
 *     tex_param[t*12 + ..] = constant: color.rgb | gradient: co, cu, cv, cuv (4 x rgb) | checker: scale
 *     tex_child[t*2 + 0..1] = checker tex0, tex1 (else -1)
 *   camera (camera.clj):
 *     cam_kind      RTMI_CAM_PINHOLE (:8) | RTMI_CAM_THINLENS (:35)
 *     cam[24]       origin, lleft, horiz, vert, u, v, w (7 x xyz), aperture, t0, t1
 */
#ifndef RTMI_H
#define RTMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTMI_OK 0
#define RTMI_E_ARG (-1)         /* bad argument / malformed scene */
#define RTMI_E_DEVICE (-2)      /* no usable gfx950 device, or a HIP call failed */
#define RTMI_E_UNSUPPORTED (-3) /* record type / option not available on the GPU path */
#define RTMI_E_NOMEM (-4)
#define RTMI_E_STATE (-5)       /* handle used after destroy, wrong context, ... */

enum { RTMI_PRIM_SPHERE = 0, RTMI_PRIM_UVSPHERE = 1, RTMI_PRIM_MOVING = 2,
       /* section 8(f3), via rtmi_scene_create_ex: */
       RTMI_PRIM_RECT_XY = 3, RTMI_PRIM_RECT_XZ = 4, RTMI_PRIM_RECT_YZ = 5, RTMI_PRIM_TRIANGLE = 6,
       /* ConstantMedium (hitable.clj:516): prim_geom = density, first boundary primitive, boundary primitive count; prim_mat =
        * its phase function (RTMI_MAT_ISOTROPIC).  The primitives of a medium's boundary come AFTER all world primitives and
        * carry RTMI_PRIM_BOUNDARY in their kind: they exist only for the medium (a record that is both in the world and a
        * boundary, scene.clj:434,466-469, is listed twice). */
       RTMI_PRIM_MEDIUM = 7, RTMI_PRIM_BOUNDARY = 16 };
enum { RTMI_XFORM_TRANSLATE = 0, RTMI_XFORM_ROTATE_Y = 1 };
enum { RTMI_MAT_LAMBERTIAN = 0, RTMI_MAT_METAL = 1, RTMI_MAT_DIELECTRIC = 2, RTMI_MAT_DIFFUSE_LIGHT = 3,
       RTMI_MAT_ISOTROPIC = 4 /* shader.clj:129, only as a ConstantMedium's phase function */ };
enum { RTMI_TEX_CONSTANT = 0, RTMI_TEX_UVGRADIENT = 1, RTMI_TEX_CHECKER = 2,
       /* section 8(f4), texture.clj:60-138: PerlinNoise (tex_param = scale), PerlinTurbulence / Marble (scale, depth),
        * FlipTextureU / FlipTextureV (tex_child[0] = wrapped texture), ImageMap (tex_param[0] = image index) */
       RTMI_TEX_PERLIN_NOISE = 3, RTMI_TEX_PERLIN_TURB = 4, RTMI_TEX_MARBLE = 5, RTMI_TEX_FLIP_U = 6, RTMI_TEX_FLIP_V = 7,
       RTMI_TEX_IMAGE = 8 };
enum { RTMI_CAM_PINHOLE = 0, RTMI_CAM_THINLENS = 1 };
enum { RTMI_F64 = 0, RTMI_F32 = 1 };             /* arithmetic the kernels compute in */
enum { RTMI_ACCEL_FLAT = 0, RTMI_ACCEL_BVH = 1 }; /* Hitlist scan (hitable.clj:15-26) | bvh-node descent (hitable.clj:97-123) */

#define RTMI_PRIM_STRIDE 9
#define RTMI_TEX_STRIDE 12
#define RTMI_TILE 8          /* framebuffer tiles are RTMI_TILE x RTMI_TILE pixels */
#define RTMI_TILE_PIXELS 64
#define RTMI_SEG_REC 12      /* doubles per logged path segment: prim, t, p.xyz, n.xyz, next dir.xyz, scattered? */

#define RTMI_FLAG_TIMING 1u  /* record HIP events around the trace kernel and its reduction (rtmi_last_trace_ms, rtmi_last_reduce_ms) */

typedef struct rtmi_ctx rtmi_ctx;
typedef struct rtmi_scene rtmi_scene;

/* ---- library / context ---------------------------------------------------------------- */
const char *rtmi_last_error(void);
const char *rtmi_backend_name(void); /* "hip-gfx950" */
int rtmi_version(void);

/* Binds a context to HIP device `device` (one process per GPU: pass LOCAL_RANK; one process for the node: one context per
 * device, see rtmi_render_multi). */
int rtmi_init(int device, uint32_t flags, rtmi_ctx **out_ctx);
int rtmi_shutdown(rtmi_ctx *ctx);
/* knobs: "accel" (RTMI_ACCEL_*; default RTMI_ACCEL_BVH -- bit-identical to the flat scan), "count_traversal" (0/1: the next
 * renders run the counting instantiation of the BVH kernel, see rtmi_last_traversal_counters), "suspend_lanes" (0..64, default 8: the
 * BVH traversal of a wave stops descending / hands the wave back when fewer lanes than this are still descending / in the tree, and the
 * parked lanes resume in the next trip; 0 = the plain loop; the image does not depend on it), "flat_below" (default 24: a scene of rectangles /
 * triangles / instances / media / f4 textures with fewer primitives than this renders through the flat scan even under RTMI_ACCEL_BVH -- same image, a
 * tree over so few primitives only costs; 0 = never; renders with "count_traversal" always walk the tree), "workspace_bytes" (sample-buffer budget, default 64 GiB, allocated as needed: a frame is rendered in as many sample passes as
 * it takes), "defer_emitters" (0/1, default 1; the image does not depend on it: in a scene of spheres whose only UVSphere light is a
 * dome with a UVGradient that reads v alone -- the cover scene's sky --, a path that ends on that light is stored as {attenuation, normal y}
 * and finished where the pixel's samples are summed, the same operations on the same operands (renders through the tree, "count_traversal"
 * off; every other render is as with 0); a sample record then holds four reals, not three.  "workspace_bytes" still counts three per sample, so a call splits into the same passes either way, and the fourth is allocated on
 * top of that budget -- within what the free-HBM clamp allows; 0: every render stores finished three-real samples; environment
 * RTMI_DEFER_EMITTERS=0/1 overrides it), "blocks_per_cu" (cap on resident trace workgroups per CU; the launch never exceeds what stays resident),
 * "scan_variant" (flat scan: 0 LDS literal, 1 LDS pipelined, 2 scalar cache, 3 scalar cache + FP32 cull = default),
 * "lds_tile_bytes" (LDS variants), "timing" (0/1 = RTMI_FLAG_TIMING); test hooks: "test_fail_next_render" (the context's next render
 * fails before launching anything), "test_fail_allocs" (its next n sample-buffer allocations fail).
 * A context owns its workspace and work queue and is not re-entrant; for several frames in flight on one GPU use one context
 * (and one stream) per frame slot. */
int rtmi_set_option(rtmi_ctx *ctx, const char *name, int64_t value);
int rtmi_device_info(rtmi_ctx *ctx, int32_t *compute_units, int32_t *lds_bytes_per_cu, int64_t *hbm_bytes, char *arch, int32_t arch_len);

/* ---- scene ------------------------------------------------------------------------------- */
/* Replaces building the world the reference's Hitlist.hit? walks (hitable.clj:15-26) and the
 * camera record get-ray reads (camera.clj:8-16,35-48): uploads the flat arrays to HBM (SoA). */
int rtmi_scene_create(rtmi_ctx *ctx,
                      int32_t n_prims, const int32_t *prim_kind, const double *prim_geom, const int32_t *prim_mat,
                      int32_t n_mats, const int32_t *mat_kind, const int32_t *mat_tex, const double *mat_param,
                      int32_t n_tex, const int32_t *tex_kind, const double *tex_param, const int32_t *tex_child,
                      int32_t cam_kind, const double *cam, rtmi_scene **out_scene);
/* The same plus the instancing records of hitable.clj:269-511, 548-581 (Cornell-box class scenes):
 *   prim_kind[i] may also be RTMI_PRIM_RECT_XY/XZ/YZ (hitable.clj:269/301/333; prim_geom = a0, b0, a1, b1, k: the two in-plane
 *   extents in the order of the record's fields, then the plane's coordinate) or RTMI_PRIM_TRIANGLE (hitable.clj:548;
 *   prim_geom = v0.xyz, v1.xyz, v2.xyz);
 *   prim_flip[i]      parity of the FlipNormals wrappers (hitable.clj:375) around primitive i;
 *   prim_xform[i*2..] first index and count of primitive i's Translate / RotateY wrappers (hitable.clj:391, 410) in the
 *                     xform table, OUTERMOST FIRST;  xform_kind[k] = RTMI_XFORM_*;
 *   xform_param[k*3..] Translate: offset.xyz | RotateY: sin-theta, cos-theta, 0 (the record's fields, hitable.clj:410).
 * Box (hitable.clj:491) flattens to its six rectangles.  ConstantMedium (hitable.clj:516-541) draws its random number inside
 * hit?: by default media are evaluated in primitive-index order with the un-narrowed (t-min, t-max) of the reference's bvh-node descent;
 * a world that IS a Hitlist holding media is declared with rtmi_scene_set_media_mode(RTMI_MEDIA_HITLIST); at most 16 media per scene.  Scenes that use
 * any of this are rendered by the FP64 kernels only (RTMI_F32 -> RTMI_E_UNSUPPORTED). */
int rtmi_scene_create_ex(rtmi_ctx *ctx,
                         int32_t n_prims, const int32_t *prim_kind, const double *prim_geom, const int32_t *prim_mat,
                         int32_t n_mats, const int32_t *mat_kind, const int32_t *mat_tex, const double *mat_param,
                         int32_t n_tex, const int32_t *tex_kind, const double *tex_param, const int32_t *tex_child,
                         int32_t cam_kind, const double *cam,
                         const int32_t *prim_flip, const int32_t *prim_xform,
                         int32_t n_xforms, const int32_t *xform_kind, const double *xform_param, rtmi_scene **out_scene);
/* The namespace-level tables of perlin.clj:6-17 as scene data (the reference fills them from the unseeded global RNG when
 * the namespace loads): vectors[256*3] = random-vectors (unit vectors), perm[3*256] = perm-x, perm-y, perm-z (each a
 * permutation of 0..255).  Required before rendering a scene that holds a Perlin texture. */
int rtmi_scene_set_perlin(rtmi_scene *scene, const double *vectors, const int32_t *perm);
/* The pixels ImageMap (texture.clj:126-133) samples: n images, wh[2*i] = width, height of image i, rgb = the images'
 * rows (top row first, RGB bytes) concatenated.  Replaces imagez load-image / get-pixel (texture.clj:76,138). */
int rtmi_scene_set_images(rtmi_scene *scene, int32_t n_images, const int32_t *wh, const uint8_t *rgb);
/* The order in which, and how often, the reference's descent calls hit? of the scene's ConstantMedium primitives per ray:
 * calls[k] = index of a RTMI_PRIM_MEDIUM primitive, n_calls <= 32.  Default: every medium once, ascending index.  (make-bvh
 * stores a lone item as bvh-node(L, L), hitable.clj:113-114, and bvh-node.hit? evaluates both children: a medium there is
 * asked twice, draws two random numbers and the nearer scattering point wins.) */
int rtmi_scene_set_media_calls(rtmi_scene *scene, int32_t n_calls, const int32_t *calls);
/* How a ConstantMedium's hit? is called (it draws its random number INSIDE hit?, hitable.clj:529, so the t-max it is handed matters):
 *   RTMI_MEDIA_DESCENT (default)  the world is a make-bvh tree: bvh-node.hit? hands both children the un-narrowed (t-min, t-max)
 *                                 (hitable.clj:99-105); the media are evaluated after the surfaces, in call order (rtmi_scene_set_media_calls);
 *   RTMI_MEDIA_HITLIST            the world is a Hitlist (nested Hitlists / Boxes / instance wrappers spliced in item order, no bvh-node
 *                                 anywhere): Hitlist.hit? hands every item the t-max narrowed by the items BEFORE it (hitable.clj:15-26), so
 *                                 a medium is evaluated at its place in the list with the closest hit so far as its t-max; the primitives
 *                                 must be in list order and every medium is called once, in ascending index order.
 * A world that mixes the two (a Hitlist holding media below a bvh-node) is not supported: the flatteners raise "unsupported on GPU path". */
enum { RTMI_MEDIA_DESCENT = 0, RTMI_MEDIA_HITLIST = 1 };
int rtmi_scene_set_media_mode(rtmi_scene *scene, int32_t mode);
/* The general form (round 4): Hitlists holding media BELOW bvh-nodes.  calls = the media call sequence as for rtmi_scene_set_media_calls; narrow_from[k] = the
 * first primitive of the Hitlist items that stand before call k's medium in its own (possibly nested) Hitlist -- Hitlist.hit? hands the medium the closest hit
 * among primitives [narrow_from[k], calls[k]) as its t-max (hitable.clj:15-26), whatever the bvh-nodes above that Hitlist do (they pass the interval on
 * un-narrowed, hitable.clj:99-105); narrow_from[k] = calls[k]: no item narrows it (a medium reached through bvh-nodes only).  The items of a Hitlist are
 * contiguous in the flattened order; calls that share a narrowing list come in list order.  Replaces both calls above for such worlds; still unsupported: a
 * bvh-node BETWEEN a narrowing Hitlist and its medium, a medium inside a medium's boundary. */
int rtmi_scene_set_media_calls_narrowed(rtmi_scene *scene, int32_t n_calls, const int32_t *calls, const int32_t *narrow_from);
/* ---- the camera of a live scene: another viewpoint or shutter without a new scene (a turntable, a fly-through, a shutter sweep, a drag of the mouse) ----
 * The promise: after either set call has succeeded, every entry that reads the scene -- rtmi_render*, the tiles, progressive, adaptive and multi forms,
 * rtmi_render_features* and the probes -- returns, BIT FOR BIT, what it returns for a scene freshly created from the same arrays (and the same
 * rtmi_scene_set_* calls) with this camera: frame, 8-bit frame, standard error, samples, features and the ray counters.  Only the traversal counters of
 * rtmi_last_traversal_counters may differ: they describe the tree, and the tree may differ (it is a conservative filter in front of the exact tests; a
 * fresh scene takes |camera origin| into the bound its boxes are inflated by, and sweeps its MovingSphere boxes over its own camera's shutter).
 * Shutter interval of a camera: RTMI_CAM_PINHOLE [0, 0] (camera.clj:16: its rays carry time 0); RTMI_CAM_THINLENS [min(t0, t1), max(t0, t1)].  The camera
 * FITS if the scene holds no RTMI_PRIM_MOVING primitive, or if its interval lies inside the interval the scene was built for (the creating camera's, or the
 * last rebuild's; rtmi_scene_camera reports it).  The origin never matters: a ray that starts beyond the tree's bound moves the box planes out itself.
 *   The camera fits: only the camera changes -- in the descriptor in HBM, in the host's mirror of it and in the arguments rtmi_scene_clone replays.  No table
 *     is allocated, freed or uploaded again, rtmi_scene_device_bytes is unchanged and the built interval stays as built.
 *   It does not fit (rtmi_scene_set_camera only): rays outside the built interval would bypass the swept bounds and test every MovingSphere exactly --
 *     correct, and ruinous -- so the call rebuilds: the trees and tables are built for the new camera from the arrays the scene keeps, uploaded beside the old
 *     ones and only then swapped in; the old ones are freed after the context's stream has been synchronised.  The Perlin tables, the images, the media call
 *     sequence (a narrowed one too) and the media mode stay.  The handle and the scene's identity (the progressive key's serial) stay; on any failure the scene
 *     is exactly as before.  *out_rebuilt (may be NULL) = 1 on this path, 0 on the other.
 * Both forms change the scene's revision on success, always (the bytes are not compared): a progressive frame started before the call is refused its
 * continuation with RTMI_E_STATE, s_first = 0 starts a new one.
 * rtmi_scene_set_camera synchronises the context's stream first, like every rtmi_scene_set_* call.
 * rtmi_scene_set_camera_stream never waits for the host: the 24 doubles and the two ints travel as the arguments of a one-wave kernel that stores them into
 * the descriptor on `stream` (rtmi_render_device's stream semantics: NULL = the context's own stream).  A render queued on that stream before the call sees
 * the old camera, one queued after it the new one.  The host's mirror changes at once: what a render decides at enqueue time (the width of its camera-ray
 * stash) agrees with what its kernels will read.  If the camera does not fit: RTMI_E_UNSUPPORTED, rtmi_last_error names both intervals, nothing changes and
 * nothing is launched.  A scene's camera belongs to one stream at a time, like the workspace: renders of the scene that are still queued on ANOTHER stream
 * when either form is called are not ordered with it.
 * Errors of the two set forms, reported before the handle is examined: cam NULL: RTMI_E_ARG; cam_kind neither RTMI_CAM_PINHOLE nor RTMI_CAM_THINLENS:
 * RTMI_E_UNSUPPORTED.  Then a bad handle: RTMI_E_STATE.  Non-finite camera values are accepted, as creation accepts them. */
int rtmi_scene_set_camera(rtmi_scene *scene, int32_t cam_kind, const double *cam, int32_t *out_rebuilt);
int rtmi_scene_set_camera_stream(rtmi_scene *scene, int32_t cam_kind, const double *cam, void *stream);
/* The camera the scene renders with now (cam_kind, cam[24]) and the shutter interval its MovingSphere bounds were built for.  Every output may be NULL.
 * Host state only: no device access. */
int rtmi_scene_camera(rtmi_scene *scene, int32_t *cam_kind, double *cam, double *built_t_lo, double *built_t_hi);
/* ---- the materials and textures of a live scene: a wall's colour, a lamp's power, a metal's fuzz, glass in place of a diffuse ball, a checker's scale ----
 * Both calls take WHOLE tables with the layout rtmi_scene_create takes (the reference's records: shader.clj:29,46,76,114,129 Lambertian, Metal, Dielectric,
 * DiffuseLight, Isotropic; texture.clj:14-133 Constant ... ImageMap) and prim_mat: n_prims entries (the scene's primitive count; the `material` field of
 * hitable.clj's records), or NULL: the assignment stays as it is.  The geometry, the instancing records and the camera are the scene's.
 * The promise: after either call has succeeded, every entry that reads the scene -- rtmi_render*, the tiles, progressive, adaptive and multi forms,
 * rtmi_render_features* and the probes -- returns, BIT FOR BIT, what it returns for a scene freshly created from the edited arrays with the same camera and the
 * same rtmi_scene_set_* calls: frame, 8-bit frame, standard error, samples, features and the ray counters, in RTMI_F64 and RTMI_F32.  It holds by
 * construction: creation and the edit pack the material tables with one function.
 * Materials and textures reach the device through eleven tables (the material records with a dielectric's precomputed 1/ri and r0, the gradient corners,
 * the kinds, texture indices and parameters of the materials, the kinds, parameters and children of the textures, the primitives' materials and their kinds
 * with the RTMI_PRIM_NEEDS_U / _V / _UV bits); the trees, the entry grid and every other table read geometry only.  The edit FITS if n_mats and n_tex are the
 * scene's and the scene keeps its kernels: a section 8(f4) texture (above RTMI_TEX_CHECKER) or a used RTMI_MAT_ISOTROPIC material neither appears in a scene
 * that the sphere kernels render nor disappears from one that had nothing else to need the EXT kernels.
 *   The edit fits: only the eleven tables are written, where they lie, with the host's mirror of them and the arguments rtmi_scene_clone and a camera rebuild
 *     replay.  No table is allocated or freed, rtmi_scene_device_bytes and rtmi_scene_tree_info are unchanged, and the traversal counters equal a fresh
 *     scene's too (the tree is untouched).  *out_rebuilt (may be NULL) = 0.
 *   It does not fit (rtmi_scene_set_materials only): the scene is rebuilt from the arrays it keeps with the edited ones in their place, as for a camera that
 *     does not fit: uploaded beside the old tables, swapped, the old ones freed after the context's stream has been synchronised.  The Perlin tables, the
 *     images, the media call sequence and the media mode stay, the handle and the scene's identity stay; on any failure the scene is exactly as before.
 *     *out_rebuilt = 1.
 * A Perlin texture without rtmi_scene_set_perlin, or an ImageMap beyond the images given, is reported when rendering (RTMI_E_STATE), as for a fresh scene.
 * Both forms change the scene's revision on success, always: a progressive or adaptive frame started before the call is refused its continuation with
 * RTMI_E_STATE, s_first = 0 starts a new one.
 * rtmi_scene_set_materials synchronises the context's stream first, like every rtmi_scene_set_* call, then copies the tables that changed.
 * rtmi_scene_set_materials_stream never waits for the host, and the caller's arrays are free again when it returns: the host packs the new tables, compares
 * them row by row with its mirror, and only the changed rows travel, as the arguments of a one-wave kernel on `stream` (rtmi_render_device's stream semantics)
 * -- one launch per batch that fits the kernel-argument space, none if nothing changed.  A render queued on that stream before the call sees the old materials,
 * one queued after it the new ones; the host's mirror changes at once.  It is for the few records an interactive edit touches: more than
 * RTMI_EDIT_STREAM_MAX_BYTES of changed rows, or an edit that does not fit: RTMI_E_UNSUPPORTED, rtmi_last_error names the reason, nothing changes and nothing
 * is launched -- rtmi_scene_set_materials does both.  The scene's tables belong to one stream at a time, like its camera.
 * Errors of the two forms, in this order: a negative count or a NULL array (prim_mat excepted): RTMI_E_ARG; a bad handle: RTMI_E_STATE; then creation's
 * checks with creation's codes -- the kind ranges (RTMI_E_UNSUPPORTED), texture, child and image indices, prim_mat out of range, a medium whose material is
 * not RTMI_MAT_ISOTROPIC (RTMI_E_ARG).  Any failure leaves the scene exactly as it was. */
#define RTMI_EDIT_STREAM_MAX_BYTES 32768 /* changed row payload one rtmi_scene_set_materials_stream call carries */
int rtmi_scene_set_materials(rtmi_scene *scene,
                             int32_t n_mats, const int32_t *mat_kind, const int32_t *mat_tex, const double *mat_param,
                             int32_t n_tex, const int32_t *tex_kind, const double *tex_param, const int32_t *tex_child,
                             const int32_t *prim_mat, int32_t *out_rebuilt);
int rtmi_scene_set_materials_stream(rtmi_scene *scene,
                                    int32_t n_mats, const int32_t *mat_kind, const int32_t *mat_tex, const double *mat_param,
                                    int32_t n_tex, const int32_t *tex_kind, const double *tex_param, const int32_t *tex_child,
                                    const int32_t *prim_mat, void *stream);
/* ---- the geometry of a live scene: a sphere dragged, a radius shrunk, a Cornell block nudged or turned, a rectangle or a triangle's vertex moved ----
 * prim_geom is the WHOLE table, n_prims rows of RTMI_PRIM_STRIDE doubles as rtmi_scene_create_ex takes it, xform_param the whole table of n_xforms rows of three
 * (a Translate's offset, a RotateY's sin and cos), or NULL: it stays.  STRUCTURE is not editable: the counts, the kinds (boundary flag included), prim_flip,
 * prim_xform and xform_kind are the scene's and no arguments of this call; another n_prims or n_xforms than the scene's is RTMI_E_ARG (a changed count or kind
 * is a new scene).  The materials and the camera are the scene's.
 * The promise: after the call has succeeded every RESULT -- frame, 8-bit frame, standard error, samples, features, probes and the ray counter, in RTMI_F64 and
 * RTMI_F32 -- is BIT FOR BIT that of a scene freshly created from the edited arrays with the same camera and rtmi_scene_set_* calls.  The closest hit does not
 * depend on the tree, so the edited scene keeps the tree it has: rtmi_last_traversal_counters and rtmi_scene_tree_info describe that tree and may differ from a
 * fresh scene's.
 * mode 0: in place if the edit fits, else a rebuild; mode 1: always a rebuild (how a host asks for a fresh tree).  The edit FITS if
 *   - the scene has no Box leaves and no media neighbourhood trees (the experiment knobs RTMI_BOX_LEAF, RTMI_MLOC);
 *   - every RTMI_PRIM_MEDIUM row is bit-equal to the scene's, and no primitive changes between boundable and not (non-finite values, a MovingSphere with
 *     time0 = time1);
 *   - every boundable world primitive's new world box (MovingSpheres: swept over the shutter interval the scene was BUILT for) has |coordinate| <= the bound
 *     the trees were built with (DevScene::bvh_obound), and every tree primitive's box lies within the trees' coordinate bound (bvh_cbound);
 *   - after displacement (below) the list of big primitives, which every ray tests exactly before the tree, holds at most 16 entries.
 * In place: the context's stream is synchronised; the geometry tables whose bytes changed (packed by the function that packs them at creation) are copied where
 * they lie, with the descriptor if its big list or a medium's fast operands changed; then the node array is REFIT on the context's stream, topology kept:
 * one launch of refit_kernel per node height, lowest first, every box the union of its children's (a leaf: the primitive's box rounded as the builder rounds
 * it; the node of a tree over one primitive keeps its empty right side).  The builder's rounding is monotone, so these are the planes it would emit for the same topology over the new boxes.  The renders queued on the
 * context's stream afterwards see the new scene; the call does not wait for the refit (a render on ANOTHER stream must: any host-form rtmi_scene_set_* call
 * synchronises the context's stream first -- the scene's tables belong to one stream at a time).  The first in-place edit after a build allocates the refit plan (node
 * indices by height) and one box per world primitive, counted by rtmi_scene_device_bytes; later edits allocate nothing.
 * DISPLACEMENT: where an entry grid was built, a primitive registered in grid cells (the layer) whose new box reaches a cell it was not registered in or
 * leaves the layer's box, and a tall primitive whose box leaves the tall primitives' box, leaves the trees -- its leaves get the empty box -- and joins the
 * big list (kept in ascending index order): one more exact test per segment, what one dragged object costs.  It is judged against the range the BUILD gave
 * the primitive, never against a later edit (shrinking and growing back stays home); once displaced, a primitive stays so until a rebuild; nothing is
 * re-classified.  Scenes without a grid never displace.
 * A rebuild goes behind the same handle like a camera's or a material edit's (the old tables serve until the swap) and forgets every displacement; so does a
 * rebuild by rtmi_scene_set_camera or rtmi_scene_set_materials.
 * out_info[4] (may be NULL) = rebuilt 0 / 1, displaced primitives now in the big list, node records refit, refit launches.
 * Success always changes the scene's revision: a progressive or adaptive frame is not continued.  Errors, in this order: a negative count, a NULL prim_geom, a
 * mode other than 0 / 1: RTMI_E_ARG; a bad handle: RTMI_E_STATE; other counts than the scene's: RTMI_E_ARG; then creation's checks of the same arrays with
 * creation's codes (a medium's density NaN or its boundary range invalid: RTMI_E_ARG).  A failed call leaves the scene, revision included, as it was. */
int rtmi_scene_set_geometry(rtmi_scene *scene, int32_t n_prims, const double *prim_geom, int32_t n_xforms, const double *xform_param,
                            int32_t mode, int32_t *out_info);
/* Device time of the refit launches of the scene's last in-place rtmi_scene_set_geometry, by events on the context's stream; waits for them.  Needs a
 * context created with RTMI_FLAG_TIMING; RTMI_E_STATE if there is no such edit since the scene's last build. */
int rtmi_scene_last_refit_ms(rtmi_scene *scene, double *out_ms);
/* HBM bytes the scene occupies (everything its creation uploaded: records, tree, tables) -- bench.py's `upload_bytes` */
int rtmi_scene_device_bytes(rtmi_scene *scene, int64_t *out_bytes);
/* The device's tree as the scene was built with it: out_info[4] = node records, depth of the deepest leaf, entry-grid cells per side (0: no grid),
 * big primitives kept out of the tree -- the four numbers rtmi_test_build_tree reports.  Host state only: no device access. */
int rtmi_scene_tree_info(const rtmi_scene *scene, int32_t *out_info);
int rtmi_scene_destroy(rtmi_scene *scene);

/* ---- the hot path --------------------------------------------------------------------------- */
/* Replaces core.clj:100-108 for the output region [x0,x1) x [y0,y1): for each pixel, ns jittered
 * samples of `color` (core.clj:17-41, depth as core.clj:20,45), mean, gamma 2, 8-bit (core.clj:52-57).
 * out_linear: (y1-y0)*(x1-x0)*3 doubles, the per-pixel mean BEFORE sqrt (for RMS parity), may be NULL;
 * out_rgb8: same shape uint8, trunc(min(255.99, 255.99*sqrt(mean))), NaN -> 0, may be NULL;
 * out_counters: {total-rays (core.clj:24), total-pixels (core.clj:47)} (metrics.clj:8-9) of the region's pixels, may be NULL.
 * Only the 8x8 tiles that intersect the region are rendered.
 * Every random draw is the next value of the counter stream keyed (seed, j*nx+i, sample). */
int rtmi_render(rtmi_scene *scene, int32_t nx, int32_t ny, int32_t ns, int32_t depth, uint64_t seed, int32_t precision,
                int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                double *out_linear, uint8_t *out_rgb8, uint64_t *out_counters);

/* Same path with every buffer resident in HBM (device pointers), launched on `stream` (a hipStream_t); asynchronous.
 * stream = NULL means the CONTEXT'S OWN stream (created hipStreamNonBlocking), NOT the HIP default stream: work the caller
 * has queued on any other stream -- including the legacy default stream, whose handle is also 0 -- is not ordered with it.
 * A caller whose buffers are produced / consumed on another stream passes that stream's handle here (for the legacy
 * default stream: hipStreamLegacy) or brackets the call with events.  A context's workspace belongs to one stream at a time.
 * d_out_linear holds doubles for both precisions. */
int rtmi_render_device(rtmi_scene *scene, int32_t nx, int32_t ny, int32_t ns, int32_t depth, uint64_t seed, int32_t precision,
                       void *d_out_linear, void *d_out_rgb8, void *d_out_counters, void *stream);

/* Tile-partitioned form for one-process-per-GPU rendering (the reference's tiled-coords,
 * core.clj:59-71, becomes 8x8 tiles dealt round-robin): renders global tiles
 * tile_first, tile_first+tile_stride, ... (row-major tile index over ceil(nx/8) x ceil(ny/8)) into
 * d_tiles_linear[k][64][3] doubles (per-pixel mean, tile-major; pixels outside the image are 0).
 * The number of local tiles is rtmi_local_tiles(nx, ny, tile_first, tile_stride). */
int rtmi_render_tiles_device(rtmi_scene *scene, int32_t nx, int32_t ny, int32_t ns, int32_t depth, uint64_t seed, int32_t precision,
                             int32_t tile_first, int32_t tile_stride,
                             void *d_tiles_linear, void *d_out_counters, void *stream);
int32_t rtmi_local_tiles(int32_t nx, int32_t ny, int32_t tile_first, int32_t tile_stride);

/* ---- progressive rendering: one frame refined over calls (a preview while it renders, a time budget, more samples later) ----
 * A context holds at most one progressive frame (two frames at once: two contexts): per-pixel running sums and noise state in HBM, the
 * cumulative counters, and the key it was started with.  rtmi_render_progressive*(..., s_first, s_count, ...) adds samples
 * [s_first, s_first + s_count) of every pixel; with k = s_first + s_count the call returns
 *   out_linear / out_rgb8: the mean over samples [0, k), BIT-IDENTICAL to what rtmi_render / rtmi_render_device return with ns = k and the same
 *                          scene, nx, ny, depth, seed, precision and region -- for F64 and F32, every scene kind, any sequence of chunk sizes and
 *                          however option "workspace_bytes" splits a call into passes (every draw is keyed by (seed, pixel, sample), not by ns,
 *                          and the sums are folded in sample order exactly as the one-shot reduction folds them);
 *   out_stderr:            one double per pixel (pixel order of out_linear): for k >= 2 the largest of the three channels' standard error of
 *                          the mean, sqrt(var_c / k), var_c the unbiased sample variance of the channel's k sample values (accumulated in double
 *                          with Welford's update whatever the precision: exactly 0 when all samples of a pixel are equal); +inf for k = 1;
 *   out_counters:          {total-rays of samples [0, k), total-pixels}, equal to rtmi_render(ns = k)'s.
 * Every output may be NULL.
 * s_first == 0 starts a new frame (any previous one is discarded).  s_first > 0 must equal the k the context holds and the key must match,
 * else RTMI_E_STATE and rtmi_last_error names what differs.  The key: the scene's identity (a creation serial: a new scene allocated at a
 * destroyed scene's address does not match), its revision (every rtmi_scene_set_* call changes it), nx, ny, depth, seed, precision and region.
 * Options the image does not depend on ("accel", "suspend_lanes", "flat_below", "scan_variant", "workspace_bytes", "blocks_per_cu", "defer_emitters") may change
 * between calls, and one-shot renders on the same context may come in between: the frame has buffers of its own.
 * A call that fails before it launches anything (argument checks, a mismatched key, the test_fail_next_render hook) leaves the frame as it
 * was; a call that fails after it launched anything drops it (k = 0): a later continuation is refused rather than allowed to produce a wrong
 * image.  s_count <= 0, s_first < 0 or s_first + s_count beyond int32: RTMI_E_ARG; the other argument errors are rtmi_render's.
 * Like the workspace, the frame belongs to one stream at a time.  RTMI_FLAG_TIMING covers progressive calls too (the "reduce" interval is the
 * fold of each pass into the frame); rtmi_shutdown frees the frame. */
/* host buffers, output region [x0,x1) x [y0,y1) as rtmi_render */
int rtmi_render_progressive(rtmi_scene *scene, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                            int32_t precision, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                            double *out_linear, uint8_t *out_rgb8, double *out_stderr, uint64_t *out_counters);
/* device buffers, the whole frame, launched on `stream` with rtmi_render_device's stream semantics; asynchronous */
int rtmi_render_progressive_device(rtmi_scene *scene, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                                   int32_t precision, void *d_out_linear, void *d_out_rgb8, void *d_out_stderr, void *d_out_counters, void *stream);
int rtmi_progressive_samples(rtmi_ctx *ctx, int32_t *samples); /* k of the context's progressive frame, 0 = none */
int rtmi_progressive_release(rtmi_ctx *ctx);                   /* drop the frame and free its buffers */

/* ---- adaptive sampling: the progressive frame stops refining 8x8 tiles whose noise is below eps ----
 * The context's one progressive frame keeps per-tile state: for every local tile t the number of samples it holds, n_t, and whether the tile
 * is still ACTIVE.  A frame started by rtmi_render_progressive is the special case where every tile is active with n_t = k.
 * rtmi_render_adaptive*(..., s_first, s_count, eps, ...) does two things, in this order:
 *   1. it adds samples [s_first, s_first + s_count) to every tile that is active when the call starts: the ordinary trace launches (the same
 *      kernel choice, pass loop and "workspace_bytes" splitting) over the compacted list of active tiles, in ascending tile order.  Retired
 *      tiles are not traced, folded or touched;
 *   2. it then retires tiles: with k = s_first + s_count an active tile is RETIRED if k >= 2 and every pixel of the tile that lies inside the
 *      image and the region passes: the value rtmi_render_progressive would report in out_stderr after k samples -- per channel
 *      sqrt((M2 / (k - 1)) / k), the resolve's own expression -- is <= eps.  It is compared as se <= eps: a NaN fails and the tile stays
 *      active.  Retirement is permanent for the life of the frame.  A tile retired by this call keeps the samples this call gave it (n_t = k).
 * Outputs, each of which may be NULL:
 *   out_linear / out_rgb8: per pixel the mean over its tile's samples [0, n_t), BIT-IDENTICAL to what rtmi_render returns for that pixel with
 *                          ns = n_t and the same scene, nx, ny, depth, seed, precision and region (every draw is keyed by (seed, pixel, sample),
 *                          never by ns: a tile that stopped at n samples holds what the one-shot render with ns = n computes for its pixels);
 *   out_stderr:            as rtmi_render_progressive's, with n_t in place of k;
 *   out_samples:           n_t per pixel, int32, pixel order of out_stderr;
 *   out_counters:          {ray segments of all samples traced into the frame so far, total-pixels of the region}.
 * s_first == 0 starts a new frame (any previous one is discarded).  s_first > 0 must equal the frame's k, the number of samples OFFERED so far
 * (rtmi_progressive_samples), and the key must match as for rtmi_render_progressive, else RTMI_E_STATE and rtmi_last_error names what differs.
 * eps is not part of the key and may change between calls; eps < 0, NaN or infinite: RTMI_E_ARG; eps == 0 retires only tiles whose samples are
 * all equal.  rtmi_render_adaptive may continue a frame that rtmi_render_progressive started.  rtmi_render_progressive with s_first > 0 on a
 * frame that has a retired tile returns RTMI_E_STATE (its "equals ns = k" promise cannot hold there) and leaves the frame untouched.  A call
 * that starts with no active tile launches no trace: RTMI_OK, k advanced, the outputs resolved.  Failures are the progressive call's: before
 * anything launched the frame stays as it was, after a launch it is dropped.  RTMI_FLAG_TIMING covers these calls; rtmi_progressive_release
 * and rtmi_shutdown free the per-tile state with the frame.  One-shot renders on the same context may come in between: the frame keeps its own
 * tile lists. */
/* host buffers, output region [x0,x1) x [y0,y1) as rtmi_render */
int rtmi_render_adaptive(rtmi_scene *scene, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, double eps,
                         int32_t depth, uint64_t seed, int32_t precision, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                         double *out_linear, uint8_t *out_rgb8, double *out_stderr, int32_t *out_samples, uint64_t *out_counters);
/* device buffers, the whole frame, launched on `stream` with rtmi_render_device's stream semantics.  Unlike rtmi_render_progressive_device this
 * call synchronises the stream once, at its end: the host needs the length of the next active list to size the next launch and to answer
 * rtmi_adaptive_status. */
int rtmi_render_adaptive_device(rtmi_scene *scene, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, double eps,
                                int32_t depth, uint64_t seed, int32_t precision,
                                void *d_out_linear, void *d_out_rgb8, void *d_out_stderr, void *d_out_samples, void *d_out_counters, void *stream);
/* tiles still active, local tiles of the frame, sum over the region's pixels of n_t; zeros without a frame.  Host state only: no device access. */
int rtmi_adaptive_status(rtmi_ctx *ctx, int32_t *active_tiles, int32_t *total_tiles, int64_t *pixel_samples);
/* The active list itself: out_count = tiles still active; with out_tiles != NULL (capacity >= that count, else RTMI_E_ARG) their global tile
 * indices (row-major over ceil(nx/8) x ceil(ny/8)), in ASCENDING order -- the order the next call traces them in.  Copies the list from the
 * device (an adaptive call has synchronised its stream when it returns).  Without a frame: 0 and RTMI_OK. */
int rtmi_adaptive_active_tiles(rtmi_ctx *ctx, int32_t capacity, int32_t *out_tiles, int32_t *out_count);

/* ---- retiring tiles by a noise map the caller supplies (a filtered estimate, a relative or display-space error, a region-of-interest mask) ----
 * rtmi_adaptive_retire*(ctx, nx, ny, noise, eps, out_retired) acts on the context's one progressive frame and only on its per-tile state: it adds
 * no samples and leaves k, every n_t, the sums, the noise state, the counters and the key as they are.
 *   noise: [ny][nx] doubles of the WHOLE frame, row 0 = top, whatever the frame's region -- the layout of rtmi_denoise's out_stderr, whose device
 *          buffer can be handed to the device form as it is.  nx and ny must be the frame's.
 * An ACTIVE tile is RETIRED if every pixel of it that lies inside the image and the frame's region passes noise <= eps.  The comparison is
 * written exactly so: a NaN fails, +inf fails, -inf and negative values pass.  Pixels outside the region (and of tiles that are not active) are
 * not read.  There is no k >= 2 rule here: the caller owns the criterion.  Retirement is permanent for the life of the frame, as above; the
 * active list stays in ascending tile order.  out_retired (may be NULL) receives the number of tiles this call retired.
 * A frame started by rtmi_render_progressive is converted exactly as the first rtmi_render_adaptive call converts it: every tile active, n_t = k.
 * Afterwards rtmi_render_adaptive* behaves as documented (it traces the tiles still active), rtmi_adaptive_status and
 * rtmi_adaptive_active_tiles reflect the result, and rtmi_render_progressive with s_first > 0 is refused with RTMI_E_STATE once a tile has
 * retired -- and still allowed if nothing has.
 * Errors: noise NULL, eps negative, NaN or infinite, nx or ny <= 0: RTMI_E_ARG, reported before the handle is examined.  No frame, or nx / ny not
 * the frame's: RTMI_E_STATE, rtmi_last_error names what differs.  A failure before anything is launched leaves the frame as it was, a failure
 * after a launch drops it.  A call on a frame with no active tile launches nothing: RTMI_OK, 0 retired. */
/* host buffer */
int rtmi_adaptive_retire(rtmi_ctx *ctx, int32_t nx, int32_t ny, const double *noise, double eps, int32_t *out_retired);
/* device buffer, launched on `stream` with rtmi_render_device's stream semantics.  Like rtmi_render_adaptive_device it synchronises the stream
 * once, at its end: the host mirrors the length of the active list. */
int rtmi_adaptive_retire_device(rtmi_ctx *ctx, int32_t nx, int32_t ny, const void *d_noise, double eps, int32_t *out_retired, void *stream);

/* ---- first-hit feature buffers: per-pixel albedo, normal, depth and coverage of a frame (what an edge-aware filter reads) ----
 * out_features: [rows][cols][RTMI_FEATURES] doubles, row 0 = top, of the region (host form) or the whole frame (device form):
 *   channels 0-2 albedo rgb, 3-5 normal xyz, 6 depth, 7 coverage.
 * Each channel is the mean over the pixel's feature samples s = 0 .. na-1.  Feature sample s is the FIRST SEGMENT of the path render sample s
 * traces: the stream keyed (seed, j*nx+i, s), the same two jitter draws and camera draws, the same hit? of the world with t-min 0.001 and
 * t-max Float/MAX_VALUE, the media evaluated as the render evaluates them (they draw from the sample's stream; a medium's scattering point is a
 * hit).  On a hit:
 *   normal   = the hit record's :normal as the reference stores it (hitable.clj) -- not flipped toward the ray; the mean is not renormalised;
 *   depth    = sqrt((p - o) . (p - o)), p the hit record's :p, o the ray's origin, the dot product folded from the left ((x x + y y) + z z), every
 *              operation correctly rounded in the precision of the call;
 *   coverage = 1;
 *   albedo   = (sample texture u v p) at the hit record's uv and p, BOTH uv coordinates evaluated (the trace kernel's shortcut for textures that
 *              do not read one is not taken): Lambertian, Metal, Isotropic: their albedo texture; DiffuseLight: its emission texture;
 *              Dielectric: (1 1 1).  No scatter draw is made.
 * On a miss all eight values are 0.  The fold is the frame's: in the precision R of the call, in sample order starting FROM sample 0, then
 * sum * (R(1) / R(na)), widened to double.
 * out_counters (may be NULL): {feature rays = pixels * na, pixels} of the region.
 * The result does not depend on options "accel", "suspend_lanes", "flat_below", "scan_variant" or on the region, and the calls do not touch the
 * context's progressive frame or its one-shot workspace.  Errors: na <= 0: RTMI_E_ARG; the others are rtmi_render's (RTMI_F32 on a mixed-kind
 * scene: RTMI_E_UNSUPPORTED). */
#define RTMI_FEATURES 8
/* host buffers, output region [x0,x1) x [y0,y1) as rtmi_render */
int rtmi_render_features(rtmi_scene *scene, int32_t nx, int32_t ny, int32_t na, uint64_t seed, int32_t precision,
                         int32_t x0, int32_t y0, int32_t x1, int32_t y1, double *out_features, uint64_t *out_counters);
/* device buffers, the whole frame, launched on `stream` with rtmi_render_device's stream semantics; asynchronous */
int rtmi_render_features_device(rtmi_scene *scene, int32_t nx, int32_t ny, int32_t na, uint64_t seed, int32_t precision,
                                void *d_out_features, void *d_out_counters, void *stream);

/* ---- edge-aware denoiser: an a-trous wavelet filter guided by the noise estimate and the feature buffers ----
 * A pure image operation in FP64 (-ffp-contract=off, no libm call in the weights): it reads no scene and no progressive frame, so it serves
 * one-shot, progressive, adaptive and multi-device frames alike.
 *   linear_in[ny][nx][3]      the frame (the mean before sqrt);
 *   stderr_in[ny][nx]         standard error of the mean per pixel (out_stderr of the progressive / adaptive calls), may be NULL;
 *   features_in[ny][nx][8]    rtmi_render_features' result, may be NULL;
 *   iterations                0 .. 8 passes; pass i = 0, 1, ... uses tap distance step = 2^i;
 *   sigma_c, _n, _a, _d       edge-stopping widths of colour, normal, albedo and depth; 0 switches the term off (decided per launch, not by arithmetic).
 * State per pixel: the colour c (3 channels) and V, the variance of the mean: V = se * se at the start (0 when stderr_in is NULL).  One pass
 * computes, for every centre pixel p, over the taps q = p + step * (dx, dy), dy = -2 .. 2 (outer loop), dx = -2 .. 2 (inner loop), with
 * h = {1/16, 1/4, 3/8, 1/4, 1/16} indexed by dy + 2 / dx + 2, E = 2^-200, and sums folded from the left in that tap order, every operation one
 * IEEE double operation as written:
 *   a tap outside the image is skipped; a tap any of whose three colour values is not finite is skipped;
 *   x = 0
 *   x = x + (((c_p - c_q)_r^2 + (c_p - c_q)_g^2) + (c_p - c_q)_b^2) / ((sigma_c * sigma_c) * (V_p + V_q) + E)    if stderr_in and sigma_c > 0
 *   x = x + (((n_p - n_q)_x^2 + (n_p - n_q)_y^2) + (n_p - n_q)_z^2) / (sigma_n * sigma_n)                        if features_in and sigma_n > 0
 *   x = x + (((a_p - a_q)_r^2 + (a_p - a_q)_g^2) + (a_p - a_q)_b^2) / (sigma_a * sigma_a)                        if features_in and sigma_a > 0
 *   x = x + ((d_p - d_q) * (d_p - d_q)) / ((sigma_d * sigma_d) * m + E),  m = d_q * d_q if d_q * d_q > d_p * d_p else d_p * d_p
 *                                                                                                                if features_in and sigma_d > 0
 *   the tap is skipped if x is NaN;    r = 1 / (1 + x);    w = (h[dy] * h[dx]) * ((r * r) * (r * r));    the tap is skipped if w is 0 or NaN;
 *   W = W + w;    S_ch = S_ch + w * c_q,ch;    T = T + (w * w) * V_q
 * and then c'_p = S_ch / W, V'_p = T / (W * W).  A centre pixel whose own colour is not finite, or for which no tap was taken (W = 0), is passed
 * through unchanged (c and V).  A pixel with se = +inf (one sample) has V = +inf: its colour term is 0 -- no colour edge -- and 0 * inf never occurs.
 * The features are not filtered.  Outputs, each may be NULL: out_linear = c after the last pass; out_rgb8 = rtmi_render's quantiser of it;
 * out_stderr = sqrt(V) after the last pass.  iterations = 0 copies linear_in and stderr_in (0 where NULL) bit for bit.
 * The passes ping-pong between two sets of planes the context owns (its denoise workspace: 8 planes of nx * ny doubles, 15 with features).
 * Errors, reported before anything is launched (and before the handle is examined): nx or ny <= 0, iterations outside 0 .. 8, a negative or NaN
 * sigma, linear_in NULL: RTMI_E_ARG. */
/* host buffers */
int rtmi_denoise(rtmi_ctx *ctx, int32_t nx, int32_t ny, const double *linear_in, const double *stderr_in, const double *features_in,
                 int32_t iterations, double sigma_c, double sigma_n, double sigma_a, double sigma_d,
                 double *out_linear, uint8_t *out_rgb8, double *out_stderr);
/* device buffers, launched on `stream` with rtmi_render_device's stream semantics; asynchronous.  The input and output buffers may be the same. */
int rtmi_denoise_device(rtmi_ctx *ctx, int32_t nx, int32_t ny, const void *d_linear_in, const void *d_stderr_in, const void *d_features_in,
                        int32_t iterations, double sigma_c, double sigma_n, double sigma_a, double sigma_d,
                        void *d_out_linear, void *d_out_rgb8, void *d_out_stderr, void *stream);

/* ---- temporal accumulation: the previous frame reprojected into a moved camera and blended with the current one ----
 * A pure image operation in FP64 (-ffp-contract=off; sqrt, floor and / are the only functions, all correctly rounded) plus two cameras: it reads no
 * scene, no progressive frame and no workspace of another call, so it serves one-shot, progressive, denoised and multi-device frames alike.  All
 * planes are [ny][nx] row-major, row 0 = top.
 *   prev_cam_kind, prev_cam[24] / cur_cam_kind, cur_cam[24]   the cameras of the history and of the current frame (rtmi_scene_create's layout).  For
 *                             both kinds only origin o, lleft l, horiz h and vert v (cam[0..11]) are read: a thin lens is reprojected through its lens
 *                             centre; aperture, u, v, w and the shutter are ignored.  Below the previous camera's are primed.
 *   prev_linear[ny][nx][3]    the history's colour;   prev_weight[ny][nx]  the samples accumulated behind it, as doubles;
 *   prev_stderr[ny][nx]       its standard error, may be NULL;   prev_features[ny][nx][8]  rtmi_render_features' result of the previous view;
 *   cur_linear, cur_stderr (may be NULL), cur_features   the same of the current frame;   cur_weight  the samples of the current frame (ns), one
 *                             scalar for all pixels (a frame with per-pixel sample counts is not served);
 *   max_history               cap of the history's weight, may be +inf;   sigma_d, sigma_n, sigma_a  tolerances of the depth, normal and albedo tests
 *                             of a tap; 0 switches the test off (decided per launch, not by arithmetic).
 * Once per call, on the host:  a = l' - o';  n = h' x v' = (h'y v'z - h'z v'y, h'z v'x - h'x v'z, h'x v'y - h'y v'x);  nn = (nx nx + ny ny) + nz nz;
 * A = (ax nx + ay ny) + az nz.  Every dot product here and below is folded from the left like these two, every cross product is written like n, and
 * every operation is one IEEE double operation as written.
 * Per pixel, column i, row y, j = ny-1-y, f = cur_features[y][i], c = cur_linear[y][i]:
 *   1. world point:   u = (i + 0.5) / nx;  v = (j + 0.5) / ny;  d = ((l + u h) + v v) - o per component;  L = sqrt(d . d);  s = f[6] / L;
 *                     P = o + s d per component.
 *   2. into the previous camera:   q = P - o';  D = q . n;  t = A / D;  reject unless t > 0 (a NaN rejects);  X = t q - a per component;
 *                     u' = ((X x v') . n) / nn;  v' = ((h' x X) . n) / nn;  fx = u' nx - 0.5;  fy = (ny - 1) - (v' ny - 0.5);
 *                     reject unless -1 < fx < nx and -1 < fy < ny;  dist = sqrt(q . q).
 *   3. taps:          x0 = floor(fx), y0 = floor(fy), ax = fx - x0, ay = fy - y0; four taps in the order (ty, tx) = (0,0), (0,1), (1,0), (1,1) at
 *                     pixel g = (x0 + tx, y0 + ty) of the history, weight b = (tx ? ax : 1 - ax) * (ty ? ay : 1 - ay).  A tap is ACCEPTED iff it
 *                     lies inside the image; b > 0; prev_features[g][7] == 1; prev_weight[g] is finite and > 0; the three values of prev_linear[g]
 *                     are finite; prev_stderr[g] (if prev_stderr is given) is not NaN;
 *                       if sigma_d > 0:  dq = prev_features[g][6], e = dq - dist, m = dq > dist ? dq : dist, (e e) <= (sigma_d sigma_d) (m m);
 *                       if sigma_n > 0:  e = f[3..5] - prev_features[g][3..5] per component, (e . e) <= sigma_n sigma_n;
 *                       if sigma_a > 0:  the same over channels 0..2 with sigma_a
 *                     (each comparison as written: a NaN fails).  Accepted taps fold from the left, starting from 0:
 *                       W = W + b;  S_ch = S_ch + b prev_linear[g][ch];  N = N + b prev_weight[g];  T = T + b (prev_stderr[g] prev_stderr[g]).
 *   4. the pixel TAKES HISTORY iff f[7] == 1, its own three colour values c are finite, it was not rejected in 2 and W != 0.
 *      It does not:   out_linear = c and out_stderr = cur_stderr, bit for bit;  out_weight = cur_weight.
 *      It does:       c_h = S / W per channel;  n_h = N / W, then n_h = max_history if n_h > max_history;  V_h = T / W;  w = n_h + cur_weight;
 *                     out_linear = (n_h c_h + cur_weight c) / w per channel;  out_weight = w;
 *                     V = ((n_h n_h) V_h + (cur_weight cur_weight) (cur_stderr cur_stderr)) / (w w);  out_stderr = sqrt(V)
 *                     (a one-sample frame has stderr +inf and gives +inf; both weights are positive, so 0 * inf does not occur).
 * Outputs, each may be NULL: out_linear [ny][nx][3]; out_rgb8 = rtmi_render's quantiser of it; out_weight [ny][nx]; out_stderr [ny][nx], written only
 * when BOTH stderr inputs are given (else passing it is RTMI_E_ARG); out_counters = {pixels, pixels that took history}.
 * The history is gathered from neighbours: no output may be the same pointer as a prev_* input.  The cur_* inputs are read pointwise: outputs may
 * alias them.  The limits are those of the inputs: depth is a mean over jittered feature samples, so pixels on a silhouette are approximate; shading
 * that depends on the view (metal, glass) and anything that moves is held back by max_history alone; pixels whose coverage is not 1 never take history.
 * Errors, reported before anything is launched and before the handle is examined (they need no device): nx or ny <= 0; a NULL camera; NULL
 * prev_linear, prev_weight, prev_features, cur_linear or cur_features; cur_weight not finite or <= 0; max_history NaN or <= 0; a negative or NaN sigma;
 * out_stderr without both stderr inputs; an output equal to a prev_* input: RTMI_E_ARG.  A camera kind other than RTMI_CAM_PINHOLE /
 * RTMI_CAM_THINLENS: RTMI_E_UNSUPPORTED.  Then a bad handle: RTMI_E_STATE. */
/* host buffers */
int rtmi_reproject(rtmi_ctx *ctx, int32_t nx, int32_t ny, int32_t prev_cam_kind, const double *prev_cam, int32_t cur_cam_kind, const double *cur_cam,
                   const double *prev_linear, const double *prev_weight, const double *prev_stderr, const double *prev_features,
                   const double *cur_linear, const double *cur_stderr, const double *cur_features, double cur_weight,
                   double max_history, double sigma_d, double sigma_n, double sigma_a,
                   double *out_linear, uint8_t *out_rgb8, double *out_weight, double *out_stderr, uint64_t *out_counters);
/* device buffers, launched on `stream` with rtmi_render_device's stream semantics; asynchronous.  The two cameras are HOST arrays: they and the
 * constants computed from them travel as kernel arguments. */
int rtmi_reproject_device(rtmi_ctx *ctx, int32_t nx, int32_t ny, int32_t prev_cam_kind, const double *prev_cam, int32_t cur_cam_kind, const double *cur_cam,
                          const void *d_prev_linear, const void *d_prev_weight, const void *d_prev_stderr, const void *d_prev_features,
                          const void *d_cur_linear, const void *d_cur_stderr, const void *d_cur_features, double cur_weight,
                          double max_history, double sigma_d, double sigma_n, double sigma_a,
                          void *d_out_linear, void *d_out_rgb8, void *d_out_weight, void *d_out_stderr, void *d_out_counters, void *stream);

/* ---- caller-supplied rays: every camera model, baker and probe the two built-in cameras are not ----
 * n = n_groups * group rays, each 7 doubles {o.xyz, d.xyz, time} in the row layout of rtmi_probe_paths; ray r of group g is row g * group + r.
 * Each ray is one path of `color` (core.clj:17-41): hit? of the world with t-min 0.001, then scatter / emitted, up to `depth`; attenuation starts
 * at 1.  The operations are rtmi_probe_paths' on the same ray, key, ctr0 and depth, bit for bit; rays are not validated (a non-finite ray yields
 * what the device functions yield for it and never runs past depth + 1 segments).
 *   keys != NULL: row k's stream is keyed keys[k].  keys == NULL: it is keyed rtmi_sample_key(seed, g, g_first + r).  Either way the stream
 *     starts at draw ctr0 (a caller that took its jitter from draws 0 and 1 of that stream passes ctr0 = 2, as a camera path continues).
 *   out_rays (may be NULL): [n][3] doubles, the radiance of each ray.
 *   out_mean: [n_groups][3] doubles.  The group's rays summed IN ROW ORDER in the precision R of the call, starting FROM the first ray (not 0 +
 *     first), then sum * (R(1) / R(count)), widened to double: the frame's fold.
 *   out_stderr: [n_groups] doubles, rtmi_render_progressive's out_stderr with "pixel" read as "group": Welford's update in double whatever the
 *     precision, the largest channel's sqrt((M2 / (count - 1)) / count); exactly 0 when all samples are equal, +inf for count == 1.
 *   out_counters (may be NULL): {segments traced by this call (the sum of the paths' segment counts = total-rays of metrics.clj), rays n}.
 *   state (may be NULL): in/out, [n_groups][RTMI_RAYS_REC] doubles, the group's running record:
 *       [0..2] the sums (in R, widened to double), [3..5] Welford's mean per channel, [6..8] Welford's M2 per channel, [9] count.
 *     g_first == 0 starts the records; g_first > 0 continues them and must equal every record's count: the host form checks this (RTMI_E_STATE,
 *     state untouched), the device form does not read back -- it is the caller's contract.  With a state, out_mean and out_stderr are those over
 *     rays [0, g_first + group) of each group, and for any split of a group's rays into consecutive chunks the mean, the stderr and the sum of
 *     the calls' counters are bit-identical to one call with all of them.  Without a state g_first only offsets the derived keys.
 * n must fit the 32-bit work items of the kernels: n <= 2^31 - 64 (else RTMI_E_ARG); n_groups == 0 succeeds and launches nothing.
 * RTMI_F32: sphere worlds only (a mixed-kind scene: RTMI_E_UNSUPPORTED), as the probes.
 * Errors, in this order: n_groups < 0, group <= 0, g_first < 0, depth < 0 or an overflow (n, g_first + group): RTMI_E_ARG; rays NULL, or
 * out_mean / out_stderr NULL with n_groups > 0: RTMI_E_ARG; a bad handle: RTMI_E_STATE; a bad precision: RTMI_E_ARG.
 * The result does not depend on the scene's camera, on options "accel", "flat_below", "suspend_lanes", "blocks_per_cu" or "workspace_bytes" (which
 * may split the call into passes of whole groups).  The calls do not touch the context's progressive or adaptive frame, nor the scene's
 * revision.  RTMI_FLAG_TIMING covers them: rtmi_last_trace_ms / rtmi_last_reduce_ms report the trace and fold intervals as for a render. */
#define RTMI_RAYS_REC 10
/* host buffers; synchronous */
int rtmi_render_rays(rtmi_scene *scene, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first,
                     const double *rays, const uint64_t *keys, uint64_t seed, uint32_t ctr0, int32_t depth,
                     double *state, double *out_mean, double *out_stderr, double *out_rays, uint64_t *out_counters);
/* every pointer a device pointer; asynchronous on `stream` with rtmi_render_device's stream semantics.  Allocates nothing once the context's
 * workspace has grown to size; without d_out_rays the per-ray radiance lives in that workspace. */
int rtmi_render_rays_device(rtmi_scene *scene, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first,
                            const void *d_rays, const void *d_keys, uint64_t seed, uint32_t ctr0, int32_t depth,
                            void *d_state, void *d_out_mean, void *d_out_stderr, void *d_out_rays, void *d_out_counters, void *stream);

/* ---- closest-hit and any-hit queries on caller-supplied rays: picking, snapping, first hits of a baker, shadow / ambient-occlusion / line-of-sight rays ----
 * n rays, each 7 doubles {o.xyz, d.xyz, time} in the row layout of rtmi_probe_hit and rtmi_render_rays; rays are not validated (a non-finite ray yields
 * what the device functions yield for it: both calls return).
 *   t_range (may be NULL): [n][2] doubles, ray k's own (t-min, t-max) -- a shadow ray ends at its light, an ambient-occlusion ray at its radius.
 *     NULL: every ray takes the scalars t_min, t_max (which are ignored otherwise).
 *   keys, ctr0: the stream a ConstantMedium draws from inside hit?.  keys == NULL: every ray is keyed 0 and starts at draw 0, as rtmi_probe_hit's
 *     (ctr0 is ignored); else ray k's stream is keyed keys[k] and starts at draw ctr0.  Scenes without media never read it.
 * rtmi_query_hits: hit? of the world (closest hit) per ray.
 *   out_hits: [n][RTMI_HIT_REC] doubles.  [0..10] = {hit?, prim, t, p.xyz, normal.xyz, u, v}: bit for bit what rtmi_probe_hit writes for ray k with that ray's
 *     (t-min, t-max) and the same stream; [11] = the hit primitive's material index.  All zeros on a miss.
 *   out_counters (may be NULL): {rays, rays that hit}.
 * rtmi_query_occluded: is ANY primitive hit within the ray's range?  n = n_groups * group rays, ray r of group g is row g * group + r (rtmi_render_rays).
 *   out_occluded (may be NULL): [n] bytes, 1 iff rtmi_query_hits would report a hit for ray k, else 0.
 *   out_count (may be NULL): [n_groups] int32, the number of occluded rays of group g (integers: exact in any order); zeroed by the call.
 *   out_counters (may be NULL): {rays, occluded rays}.
 *   Only the flag is promised, and it does not depend on the order primitives are visited in.  A primitive ACCEPTS a ray when it has a root in
 *   (t-min, t-max): for rectangles and triangles t-min <= t <= t-max (hitable.clj:278, 564), for spheres t-min < t < t-max, the second root taken when
 *   the first is not above t-min (hitable.clj:195-203).  The closest-hit search hands every primitive the closest t so far as its t-max
 *   (hitable.clj:20), which is the INITIAL t-max until the first acceptance and afterwards only rejects candidates that are not closer: it reports a
 *   hit iff some primitive accepts the ray against the initial t-max.  The any-hit search tests primitives against the initial t-max and leaves at the
 *   first acceptance, so whichever primitive it meets first it reports the same flag.  The arithmetic of a test does not depend on the order either: the
 *   sphere roots' division takes its fast form (make_quot) by the ray's own a, t-min and t-max.  The conservative boxes of the trees are cut at the same
 *   t-max in both searches.  Worlds that hold a ConstantMedium: with media_seq == 0 the media are asked first, against the caller's interval as the
 *   closest-hit search asks them, and the surfaces leave early; the Hitlist forms (RTMI_MEDIA_HITLIST / _NARROWED), whose media see the surfaces'
 *   closest hit, run the closest-hit search unchanged and report its flag.
 * n <= 2^31 - 64 (else RTMI_E_ARG); n == 0 / n_groups == 0 succeeds and launches nothing.  RTMI_F32: sphere worlds only (RTMI_E_UNSUPPORTED), as the probes.
 * Errors, in this order: n < 0, n_groups < 0, group <= 0 or an overflow of n: RTMI_E_ARG; rays NULL, or out_hits NULL, with n > 0: RTMI_E_ARG; a bad
 * handle: RTMI_E_STATE; a bad precision: RTMI_E_ARG.
 * Results do not depend on options "accel", "flat_below", "suspend_lanes", "scan_variant", "blocks_per_cu" or "workspace_bytes".  The calls touch neither
 * the context's progressive or adaptive frame nor the scene's revision.  RTMI_FLAG_TIMING covers them: the trace interval of rtmi_last_trace_ms is the
 * query kernel (the fold interval is empty).  Option "count_traversal" = 1: the FP64 sphere-tree kernels of both calls add their AABB and primitive
 * tests to what rtmi_last_traversal_counters reads; every other family (flat scans, RTMI_F32, mixed-kind scenes) ignores the option for these calls and
 * leaves those counters at zero. */
#define RTMI_HIT_REC 12
/* host buffers; synchronous */
int rtmi_query_hits(rtmi_scene *scene, int32_t precision, int32_t n, const double *rays, const double *t_range, double t_min, double t_max,
                    const uint64_t *keys, uint32_t ctr0, double *out_hits, uint64_t *out_counters);
/* every pointer a device pointer; asynchronous on `stream` with rtmi_render_device's stream semantics.  Allocates nothing once the context's
 * workspace has grown to size. */
int rtmi_query_hits_device(rtmi_scene *scene, int32_t precision, int32_t n, const void *d_rays, const void *d_t_range, double t_min, double t_max,
                           const void *d_keys, uint32_t ctr0, void *d_out_hits, void *d_out_counters, void *stream);
/* host buffers; synchronous */
int rtmi_query_occluded(rtmi_scene *scene, int32_t precision, int32_t n_groups, int32_t group, const double *rays, const double *t_range,
                        double t_min, double t_max, const uint64_t *keys, uint32_t ctr0,
                        uint8_t *out_occluded, int32_t *out_count, uint64_t *out_counters);
/* device buffers, as rtmi_query_hits_device */
int rtmi_query_occluded_device(rtmi_scene *scene, int32_t precision, int32_t n_groups, int32_t group, const void *d_rays, const void *d_t_range,
                               double t_min, double t_max, const void *d_keys, uint32_t ctr0,
                               void *d_out_occluded, void *d_out_count, void *d_out_counters, void *stream);

/* ---- occlusion rays generated on the device: ambient occlusion, shadow rays, lines of sight from points the device already holds ----
 * The points are rtmi_query_hits' records: hits = [n_points][RTMI_HIT_REC], rec = one of them.  Item m = g * n_dirs + k (g * n_targets + k) is ray k of
 * point g; the any-hit query of rtmi_query_occluded runs over the n_points * n_dirs (n_targets) items with one group per point, but a lane builds its ray
 * in registers from its point's record instead of reading seven doubles.  Every ray is built in FP64 whatever the precision and is then converted as a
 * ray read from memory is, so RTMI_F32 differs from RTMI_F64 exactly where it does in rtmi_query_occluded.  The rays' streams (what a ConstantMedium
 * draws from) are keyed 0, as with keys == NULL there.
 *   view (may be NULL): [n_points][7] doubles, the ray that found each point (what rtmi_query_hits was given).
 *   out_occluded (may be NULL): [n] bytes; out_count (may be NULL): [n_points] int32, zeroed by the call; out_counters (may be NULL): {rays generated,
 *     occluded rays}.  A point that yields no ray (below) traces nothing: its flags and its count are 0 and it adds nothing to the counters.
 *   out_rays (may be NULL): [n][7] doubles, the rays as generated; the rows of a point that yields no ray are zeros.
 *
 * THE HEMISPHERE RULE (rtmi_occlusion_hemisphere): n_dirs cosine-weighted directions about each point's normal, by Malley's method driven by the
 * reference's rand-in-unit-disk rejection loop (util.clj:32-41) -- built from + - * / sqrt alone, so a host restates it bit for bit (no cos, no sin).
 * Every product, sum and quotient below is one IEEE double operation in the order written; dot3(a, b) = (ax*bx + ay*by) + az*bz.
 *   1. p = rec[3:6], n = rec[6:9].  The point yields no ray if rec[0] == 0, if any of the six values is not finite, or if dot3(n, n) is not > 0.
 *   2. Side: with a view array, w = view[g][3:6]; if dot3(n, w) > 0, negate each component of n.  Without one, n stays as it is.  The ray's time is
 *      view[g][6], or the call's `time` argument without a view array.
 *   3. nn = n / sqrt(dot3(n, n)), component by component.
 *   4. Tangent: if |nn.x| < 0.5 then t = (+0.0, -nn.z, nn.y), else t = (nn.z, +0.0, -nn.x).  Then t = t / sqrt(dot3(t, t)), component by component.
 *   5. b = (nn.y*t.z - nn.z*t.y, nn.z*t.x - nn.x*t.z, nn.x*t.y - nn.y*t.x).
 *   6. Disk point: the stream is keyed rtmi_sample_key(seed, g, first + k) and starts at draw 0.  Candidate c is (x, y) = (2*u(2c) - 1, 2*u(2c+1) - 1),
 *      u(d) = the FP64 uniform of draw d (the top 53 bits of the draw, times 2^-53).  Take the first candidate for which (x*x + y*y) + 0*0 >= 1 is false.
 *   7. z = sqrt(1 - (x*x + y*y)).  Direction = (x*t + y*b) + z*nn per component.  Origin = p.
 *   Any split of a point's directions over `first` therefore gives the rays of one call.
 * THE TARGETS RULE (rtmi_occlusion_targets): origin p, direction targets[k] - p per component (targets = [n_targets][3] doubles), time as in step 2.
 *   "No ray" is as in step 1, but the normal is not read.  The t-range is the call's scalars: "up to the light" is (0.001, 1 - 0.001).
 * rtmi_ambient_occlusion: the whole pass for an nx x ny view of the scene's camera on one stream, without a host round trip and without a buffer of
 *   nx * ny * n_dirs rays.  (a) the closest hits (t-range (0.001, FLT_MAX)) of the pixel-centre rays, pixel m = j * nx + i row-major from the top (j = 0):
 *   origin cam[0:3], direction ((lleft + horiz*u) + vert*v) + (-origin) per component with u = (i + 1/2) / nx, v = ((ny - 1 - j) + 1/2) / ny, time 0 for
 *   the pinhole camera and t0 for the thin lens -- built on the device from the camera the scene holds there, so the call follows
 *   rtmi_scene_set_camera_stream in stream order; (b) the hemisphere rule over those records with the pixel-centre rays as the view array, directions
 *   [first, first + n_dirs), t-range (0.001, radius); (c) out_visibility[m] = 1 - count[m] / n_dirs (doubles), and 1 where the primary ray missed.
 *   out_visibility: [ny * nx] doubles; out_count (may be NULL): [ny * nx] int32 occluded directions of this call -- with `first` a caller accumulates
 *   directions over calls; out_hits (may be NULL): [ny * nx][RTMI_HIT_REC], the records of (a); out_counters (may be NULL): those of (b).
 * n_points * n_dirs, n_points * n_targets, nx * ny * n_dirs <= 2^31 - 64 (else RTMI_E_ARG); n_points == 0 (nx * ny == 0) succeeds and launches nothing.
 * RTMI_F32: sphere worlds only (RTMI_E_UNSUPPORTED), as the queries.
 * Errors, in this order: n_points < 0 (nx, ny < 0), n_dirs / n_targets <= 0, first < 0, radius not > 0, or an overflow: RTMI_E_ARG; hits, targets or
 * out_visibility NULL with work to do: RTMI_E_ARG; a bad handle: RTMI_E_STATE; a bad precision: RTMI_E_ARG.
 * Options, frames, revision and RTMI_FLAG_TIMING: as the queries (rtmi_ambient_occlusion's trace interval is its two query launches). */
/* host buffers; synchronous */
int rtmi_occlusion_hemisphere(rtmi_scene *scene, int32_t precision, int32_t n_points, const double *hits, const double *view, int32_t n_dirs, int32_t first,
                              uint64_t seed, double time, double t_min, double t_max,
                              uint8_t *out_occluded, int32_t *out_count, double *out_rays, uint64_t *out_counters);
/* every pointer a device pointer; asynchronous on `stream` with rtmi_render_device's stream semantics.  Allocates nothing once the context's
 * workspace has grown to size. */
int rtmi_occlusion_hemisphere_device(rtmi_scene *scene, int32_t precision, int32_t n_points, const void *d_hits, const void *d_view, int32_t n_dirs,
                                     int32_t first, uint64_t seed, double time, double t_min, double t_max,
                                     void *d_out_occluded, void *d_out_count, void *d_out_rays, void *d_out_counters, void *stream);
/* host buffers; synchronous */
int rtmi_occlusion_targets(rtmi_scene *scene, int32_t precision, int32_t n_points, const double *hits, const double *view, int32_t n_targets,
                           const double *targets, double time, double t_min, double t_max,
                           uint8_t *out_occluded, int32_t *out_count, double *out_rays, uint64_t *out_counters);
/* device buffers, as rtmi_occlusion_hemisphere_device */
int rtmi_occlusion_targets_device(rtmi_scene *scene, int32_t precision, int32_t n_points, const void *d_hits, const void *d_view, int32_t n_targets,
                                  const void *d_targets, double time, double t_min, double t_max,
                                  void *d_out_occluded, void *d_out_count, void *d_out_rays, void *d_out_counters, void *stream);
/* host buffers; synchronous */
int rtmi_ambient_occlusion(rtmi_scene *scene, int32_t precision, int32_t nx, int32_t ny, int32_t n_dirs, int32_t first, double radius, uint64_t seed,
                           double *out_visibility, int32_t *out_count, double *out_hits, uint64_t *out_counters);
/* every pointer a device pointer; asynchronous on `stream`.  Allocates nothing once the context's workspace has grown to size; without d_out_hits /
 * d_out_count the records and the counts live in that workspace. */
int rtmi_ambient_occlusion_device(rtmi_scene *scene, int32_t precision, int32_t nx, int32_t ny, int32_t n_dirs, int32_t first, double radius, uint64_t seed,
                                  void *d_out_visibility, void *d_out_count, void *d_out_hits, void *d_out_counters, void *stream);

/* ---- direct lighting from first hits: the scene's area lights sampled on the device (a lit preview, a lightmap's direct term) ----
 * THE LIGHTS.  rtmi_scene_lights lists, in primitive order, the primitives a light sample can be placed on.  A primitive is ELIGIBLE when
 *   - its kind is RTMI_PRIM_SPHERE or RTMI_PRIM_UVSPHERE with radius > 0, or RTMI_PRIM_RECT_XY / XZ / YZ with both extents non-zero (a1 != a0, b1 != b0);
 *   - it does not carry RTMI_PRIM_BOUNDARY;
 *   - its Translate / RotateY chain is empty (FlipNormals wrappers do not matter: DiffuseLight's emitted is two-sided, shader.clj:118);
 *   - its material is RTMI_MAT_DIFFUSE_LIGHT and that material's texture is RTMI_TEX_CONSTANT.
 * Everything else -- a MovingSphere, a triangle, an instanced lamp, a gradient or image emitter such as the cover scene's sky dome -- is simply not a light
 * for these calls; it is no error, and it still occludes and still shows its emission where a primary ray of rtmi_render_direct hits it.
 * The list is read from the host-side tables the scene keeps, at call time: it follows every rtmi_scene_set_materials* and rtmi_scene_set_geometry call made
 * before.  out_prims: `capacity` entries (may be NULL with capacity 0), the first min(count, capacity) eligible primitives; *out_count: all of them.
 * Host state only: no device access.  Errors: capacity < 0, out_count NULL, out_prims NULL with capacity > 0: RTMI_E_ARG; a bad handle: RTMI_E_STATE.
 * rtmi_test_scene_lights: test hook, host code only (no device, no handle): the same function over the flat arrays (prim_xform may be NULL: no chains).
 *
 * THE ITEMS.  Points are rtmi_query_hits' records, as for the occlusion calls above.  Item m = (g * n_samples + k) * n_lights + l is sample k of point g
 * towards light l; a point's group is its n_samples * n_lights consecutive items.  light_prims (a HOST array in both forms): the n_lights primitives to
 * sample, each eligible (else RTMI_E_ARG), at most RTMI_DIRECT_MAX_LIGHTS; NULL: all eligible primitives, n_lights is then not read.  The light table --
 * per light {kind, 5 geometry doubles, area, Le.rgb}, Le = the constant texture's colour -- travels in stream order as the arguments of a one-wave kernel:
 * the host is never waited for.
 * THE LIGHT RULE, operation by operation as the hemisphere rule: every product, sum, difference and quotient is one IEEE double operation in the order written,
 * only + - * / sqrt occur, dot3(a, b) = (ax*bx + ay*by) + az*bz.
 *   1. Steps 1 - 3 of the hemisphere rule give p, the viewer-side unit normal nn, the ray's time and "the point yields no ray".  With lambert_only != 0 a point
 *      also yields no ray unless rec[11] is a material index of the scene and mat_kind[rec[11]] == RTMI_MAT_LAMBERTIAN.
 *   2. The stream of item (g, k, l) is keyed rtmi_sample_key(seed, g * n_lights + l, first + k) and starts at draw 0; u(d) = the FP64 uniform of draw d.
 *   3. Rectangle light (prim_geom = a0, b0, a1, b1, kk): the in-plane point (a0 + u(0)*(a1 - a0), b0 + u(1)*(b1 - b0)) with kk on the axis, i.e. q = (a, b, kk)
 *      for RTMI_PRIM_RECT_XY, (a, kk, b) for RECT_XZ, (kk, a, b) for RECT_YZ; s = the axis' unit vector (0, 0, 1) / (0, 1, 0) / (1, 0, 0);
 *      area = |(a1 - a0)*(b1 - b0)|.
 *   4. Sphere light (c, r): take the disk point (x, y) of hemisphere-rule step 6 from this stream, S = x*x + y*y, root = sqrt(1 - S),
 *      s = ((2*x)*root, (2*y)*root, 1 - 2*S) (Marsaglia: uniform on the sphere), q = c + r*s per component, area = FOURPI*(r*r), FOURPI = 0x1.921fb54442d18p+3.
 *      With e = p - c: if dot3(e, e) > r*r and dot3(s, d) > 0 (d of step 5) the item yields no ray -- the far side seen from outside; a point inside the sphere
 *      (under a constant sky dome) sees all of it.
 *   5. d = q - p per component, d2 = dot3(d, d), cp = dot3(nn, d), cl = |dot3(s, d)|.  The item yields no ray unless d2 > 0, cp > 0 and cl > 0 (a NaN fails).
 *      w = ((cp*cl) / (d2*d2)) * area: both cosines and the inverse square in one quotient, no sqrt.
 *   6. The ray: origin p, direction d, the time of step 1, t-range (0.001, 1 - 0.001) -- "up to the light": the light's own surface at t = 1 is outside it.
 *   7. After the any-hit search the item's contribution is three doubles: Le * w per channel if the ray was built and is not occluded, else +0.0.
 * Rays and weights are FP64 whatever the precision; RTMI_F32 differs from RTMI_F64 exactly where rtmi_query_occluded does.
 * THE FOLD.  One lane per point sums the point's contributions in item order in double, starting FROM the first item (not 0 + first), then
 * E = sum * (1.0 / (double)samples), samples = every sample k taken so far, those that built no ray included.  state (may be NULL): [n_points][RTMI_DIRECT_REC]
 * doubles {sum.rgb, samples}, read when first > 0 and written back: it continues a point over calls under rtmi_render_rays' contract -- any split of a point's
 * samples into consecutive chunks gives the bits of one call (the host form checks state[g][3] == first: RTMI_E_STATE).  Without a state samples = n_samples.
 * The contributions live in the context's workspace, 24 bytes per item, in passes of whole points under option "workspace_bytes"; with out_contrib the call
 * is one pass into it.
 *   out_irradiance: [n_points][3]; out_contrib (may be NULL): [items][3]; out_occluded (may be NULL): [items] bytes; out_rays (may be NULL): [items][7], zeros
 *   where no ray was built; out_counters (may be NULL): {rays built, occluded rays}.
 * Zero lights (an empty list, or NULL and nothing eligible) succeeds: without a state it writes zeros to out_irradiance and out_counters and launches
 * nothing (rtmi_render_direct: none of the light passes).  With a state, in the host and the device forms alike, the fold runs over groups of no items:
 * every sample counts as one that built no ray -- the sums carry over (zeros when first == 0), samples becomes first + n_samples and
 * E = sum * (1.0 / samples), so a state split over calls continues on a scene without lights as on any other.  n_points == 0 succeeds and does nothing.
 * rtmi_render_direct: the whole pass for an nx x ny view on one stream, as rtmi_ambient_occlusion: (a) its first hits of the pixel-centre rays; (b) the light
 *   rule over those records with the pixel-centre rays as the view, all eligible lights, lambert_only = 1; (c) the resolve, per pixel: a first hit on
 *   RTMI_MAT_DIFFUSE_LIGHT: its texture at the record's (u, v, p) (Texture.sample, whatever the texture); on RTMI_MAT_LAMBERTIAN: (albedo * E) * INV_PI per
 *   channel, albedo = its texture at the record, INV_PI = 0x1.45f306dc9c883p-2; anything else, or a miss: zeros (the reference's black miss; specular
 *   transport is not direct light).  The textures are evaluated in the call's precision, E and the product in double.  out_rgb8 (may be NULL): the frame's
 *   quantiser of out_linear (sqrt, x 255.99, min, trunc, NaN -> 0).  out_linear: [ny * nx][3], row 0 = top; out_hits (may be NULL): the records of (a);
 *   state (may be NULL): [ny * nx][RTMI_DIRECT_REC]; out_counters (may be NULL): those of (b).
 * Errors, in this order: n_points < 0 (nx, ny < 0), n_samples <= 0, first < 0, n_lights < 0 or > RTMI_DIRECT_MAX_LIGHTS with a list: RTMI_E_ARG; hits,
 * out_irradiance (out_linear) NULL with work to do: RTMI_E_ARG; a bad handle: RTMI_E_STATE; a bad precision: RTMI_E_ARG; RTMI_F32 on a mixed-kind scene:
 * RTMI_E_UNSUPPORTED; rtmi_render_direct* only, whose resolve samples textures: a Perlin texture without rtmi_scene_set_perlin, or an ImageMap beyond the
 * images given: RTMI_E_STATE, as rtmi_render; a listed primitive that is out of range or not eligible, more than RTMI_DIRECT_MAX_LIGHTS eligible primitives without a list, more than
 * 2^31 - 64 items: RTMI_E_ARG.  A failed call launches nothing.  Options, frames, revision and RTMI_FLAG_TIMING: as the occlusion calls (neither entry
 * touches the progressive or adaptive frame or the scene's revision; the trace interval covers the query launches, the fold interval the fold). */
#define RTMI_DIRECT_REC 4         /* doubles per point of a direct-lighting state: sum rgb, samples */
#define RTMI_DIRECT_MAX_LIGHTS 32 /* lights one call samples */
int rtmi_scene_lights(rtmi_scene *scene, int32_t capacity, int32_t *out_prims, int32_t *out_count);
int rtmi_test_scene_lights(int32_t n_prims, const int32_t *prim_kind, const double *prim_geom, const int32_t *prim_mat,
                           int32_t n_mats, const int32_t *mat_kind, const int32_t *mat_tex, int32_t n_tex, const int32_t *tex_kind,
                           const int32_t *prim_xform, int32_t capacity, int32_t *out_prims, int32_t *out_count);
/* host buffers; synchronous */
int rtmi_direct_irradiance(rtmi_scene *scene, int32_t precision, int32_t n_points, const double *hits, const double *view, int32_t n_lights,
                           const int32_t *light_prims, int32_t n_samples, int32_t first, uint64_t seed, double time, int32_t lambert_only, double *state,
                           double *out_irradiance, double *out_contrib, uint8_t *out_occluded, double *out_rays, uint64_t *out_counters);
/* every d_ pointer a device pointer (light_prims stays a host array); asynchronous on `stream` with rtmi_render_device's stream semantics.  Allocates nothing
 * once the context's workspace has grown to size. */
int rtmi_direct_irradiance_device(rtmi_scene *scene, int32_t precision, int32_t n_points, const void *d_hits, const void *d_view, int32_t n_lights,
                                  const int32_t *light_prims, int32_t n_samples, int32_t first, uint64_t seed, double time, int32_t lambert_only,
                                  void *d_state, void *d_out_irradiance, void *d_out_contrib, void *d_out_occluded, void *d_out_rays, void *d_out_counters,
                                  void *stream);
/* host buffers; synchronous */
int rtmi_render_direct(rtmi_scene *scene, int32_t precision, int32_t nx, int32_t ny, int32_t n_samples, int32_t first, uint64_t seed, double *state,
                       double *out_linear, uint8_t *out_rgb8, double *out_hits, uint64_t *out_counters);
/* every pointer a device pointer; asynchronous on `stream`; without d_out_hits the records live in the context's workspace */
int rtmi_render_direct_device(rtmi_scene *scene, int32_t precision, int32_t nx, int32_t ny, int32_t n_samples, int32_t first, uint64_t seed, void *d_state,
                              void *d_out_linear, void *d_out_rgb8, void *d_out_hits, void *d_out_counters, void *stream);

/* ---- path tracing with next-event estimation on caller-supplied rays: rtmi_render_rays whose Lambertian vertices also sample the area lights ----
 * rtmi_render_rays' arguments plus the lights of rtmi_direct_irradiance (n_lights, light_prims: a HOST array in both forms, each entry eligible; NULL: all
 * eligible primitives of rtmi_scene_lights, n_lights is then not read; more than RTMI_DIRECT_MAX_LIGHTS: RTMI_E_ARG).  Groups, g_first, the RTMI_RAYS_REC
 * state, out_mean, out_stderr and out_rays keep rtmi_render_rays' contract: any split of a group into consecutive chunks gives the bits of one call.
 * THE NEE RULE.  The reference's Lambertian scatter p + n + b (b uniform in the unit ball) is not cosine-weighted: its directions have the density
 * 2 cos^3 / pi about the record's normal, and the reference multiplies by the albedo and nothing else.  A light-sampled path has the expectation of
 * rtmi_render_rays for every scene and depth only if its direct term uses that lobe (rtmi_render_direct's albedo * E / pi is another estimator and stays).
 * One path per ray.  The path's own stream, its rays, hits, scatters and segment count are rtmi_render_rays' for the same ray, key, ctr0 and depth, bit for
 * bit: the light samples draw from other keys.  K = the path's key, j = the 0-based index of the segment whose hit is the vertex, nl = the number of
 * sampled lights (nl >= 1).  Every product, sum, difference and quotient is one IEEE double operation in the order written.
 *   1. A light sample is taken at exactly the vertices where a RTMI_MAT_LAMBERTIAN scatter happens (the depth left is > 0, core.clj's (and (pos? depth)
 *      (scatter ...))), and nowhere else.
 *   2. The light: l = min((int)(u * nl), nl - 1), u = the FP64 uniform of draw 0 of the stream keyed rtmi_sample_key(K, j, 1).
 *   3. The sample: steps 3 - 5 of the light rule with the stream keyed rtmi_sample_key(K, j, 0), p = the hit point, the normal THE RECORD'S AS IT IS
 *      (normalised by step 3 of the hemisphere rule; no viewer-side flip: the reference scatters about the record's normal whatever side the ray came
 *      from), the time the path ray's.  d, d2, cp, cl, the far-side rule, the three "no ray" conditions and the t-range (0.001, 1 - 0.001) are unchanged;
 *      a vertex whose p or normal is not finite, or whose normal has no length, builds no ray either (step 1 of the hemisphere rule).
 *   4. The weight: w = ((((cp*cp)*(cp*cl)) / ((d2*d2)*d2)) * area) * TWO_INV_PI, TWO_INV_PI = 0x1.45f306dc9c883p-1.
 *   5. The any-hit search of rtmi_query_occluded runs on that ray (its stream keyed 0).  If it finds nothing, accum.c = accum.c + (double)T.c * ((Le.c * w) *
 *      (double)nl) per channel; contributions are added in vertex order, accum starts at +0.0, T = the path's attenuation AFTER this vertex's albedo, in
 *      the call's precision.
 *   6. The path's closing emission (atten * emitted) is dropped when the previous vertex took a light sample (step 1) AND the emitter's primitive is one of
 *      the sampled lights; otherwise it is kept: a primary ray, a ray after metal, glass or a vertex with depth 0, and every emitter that is not a sampled
 *      light (a gradient dome, a triangle, an instanced lamp, an unlisted lamp).
 *   7. radiance.c = accum.c + (double)emit.c  (emit = +0.0 where dropped).
 * nl == 0 (an empty list, or NULL and nothing eligible): the call IS rtmi_render_rays: every emission is kept and the two shadow-ray counters are zeros.
 * A scene that holds a ConstantMedium: RTMI_E_UNSUPPORTED, nothing is launched (no transmittance along shadow rays).  RTMI_F32: sphere worlds only, as
 * rtmi_render_rays; shadow rays and weights are FP64 whatever the precision, as in the light rule.
 *   out_counters (may be NULL): FOUR values {segments, rays, shadow rays built, shadow rays occluded}.
 * Errors, in this order: rtmi_render_rays' own, in their order; n_lights < 0 or > RTMI_DIRECT_MAX_LIGHTS with a list: RTMI_E_ARG; (n_groups == 0 succeeds
 * here); a ConstantMedium: RTMI_E_UNSUPPORTED; a listed primitive that is out of range or not eligible, more than RTMI_DIRECT_MAX_LIGHTS eligible
 * primitives without a list: RTMI_E_ARG.  A failed call launches nothing.  Options, frames, revision and RTMI_FLAG_TIMING: as rtmi_render_rays.
 * rtmi_probe_paths_nee: rtmi_probe_paths' sibling, one path per thread through the same device functions.  log (may be NULL): [n][max_seg][RTMI_NEE_REC]
 *   doubles per logged vertex: [0..11] RTMI_SEG_REC's values; [12] the light-sample state: 0 none at this vertex, 1 built and unoccluded, 2 built and
 *   occluded, 3 a light-sampled vertex that built no ray; [13] l; [14..16] d; [17] w (zeros where no ray is built); [18..20] T; [21..23] the contribution
 *   added (zeros unless the state is 1).  out_rgb: [n][3] the radiance of step 7; out_nseg (may be NULL): the segment counts; out_dropped (may be NULL):
 *   [n] int32, 1 where step 6 dropped the closing emission; out_nlog (may be NULL): the logged vertices per path. */
#define RTMI_NEE_REC 24
/* host buffers; synchronous */
int rtmi_render_rays_nee(rtmi_scene *scene, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first,
                         const double *rays, const uint64_t *keys, uint64_t seed, uint32_t ctr0, int32_t depth,
                         int32_t n_lights, const int32_t *light_prims,
                         double *state, double *out_mean, double *out_stderr, double *out_rays, uint64_t *out_counters);
/* every d_ pointer a device pointer (light_prims stays a host array); asynchronous on `stream` with rtmi_render_device's stream semantics */
int rtmi_render_rays_nee_device(rtmi_scene *scene, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first,
                                const void *d_rays, const void *d_keys, uint64_t seed, uint32_t ctr0, int32_t depth,
                                int32_t n_lights, const int32_t *light_prims,
                                void *d_state, void *d_out_mean, void *d_out_stderr, void *d_out_rays, void *d_out_counters, void *stream);
int rtmi_probe_paths_nee(rtmi_scene *scene, int32_t precision, int32_t n, const double *rays, const uint64_t *keys, uint64_t ctr0, int32_t depth,
                         int32_t n_lights, const int32_t *light_prims, double *out_rgb, uint64_t *out_nseg, int32_t *out_dropped,
                         double *log, int32_t max_seg, int32_t *out_nlog);

/* ---- multiple importance sampling for the light-sampled paths: the light sample and the scatter share each lamp's emission ----
 * The NEE siblings' arguments plus light_choice behind light_prims: 0 = the light is picked uniformly, 1 = by power; anything else is RTMI_E_ARG.
 * A light sample's w carries the inverse square of area sampling and is unbounded beside a lamp; the path's own scatter finds that lamp with the
 * density 2 cos^3 / pi, and the ratio of the two densities at one point is x = p_scatter / p_light = w * q, q = 1 / (the pick's probability).  The balance
 * heuristic gives the light sample the share m = x / (1 + x) and the closing emission the share of the same form at the point the scatter found, so
 * every contribution is bounded by T * Le and the expectation is rtmi_render_rays'.
 * THE MIS RULE, operation by operation as the NEE rule: every product, sum, difference and quotient is one IEEE double operation in the order written,
 * only + - * / sqrt occur, dot3(a, b) = (ax*bx + ay*by) + az*bz.  Where nothing else is said the NEE rule holds.
 *   1. Vertices: light samples are taken at the NEE rule's vertices (its step 1).  The path's own stream, rays, hits, scatters and segment count stay
 *      rtmi_render_rays' bit for bit.
 *   2. The light.  light_choice 0: the NEE rule's step 2, and q_l = (double)nl for every light.  light_choice 1: omega_l = area_l * ((Le.r + Le.g) +
 *      Le.b), C_l = the running sum of omega in list order (C_0 = omega_0, C_l = C_(l-1) + omega_l), W = C_(nl-1); l = the first index with u * W < C_l,
 *      else nl - 1, with the same draw u; q_l = W / omega_l.  If W is not finite and > 0 the call behaves as light_choice 0.  A light with omega_l = 0
 *      is never picked, and for step 7 it does not count as a sampled light: its emission is kept whole.  omega, C and q are computed on the host and
 *      travel with the light table.
 *   3. The sample, its ray and w: the NEE rule's steps 3 and 4, unchanged.
 *   4. The weight: x = w * q_l, m = x / (1.0 + x); if x is +inf, m = 1.0.  (A vertex that builds no ray has w = 0: x and m are computed all the same.)
 *   5. The contribution: if the any-hit search finds nothing, accum.c = accum.c + (double)T.c * (Le.c * m) per channel.
 *   6. The lobe value, at the same vertex, whether or not a shadow ray was built: D = the scattered ray's direction as doubles, nn = the step-3
 *      normalised record normal, a = dot3(nn, D), DD = dot3(D, D); g = ((a*a)*a) / ((DD*DD)*DD) if the vertex is valid (step 3's finiteness test of p and
 *      the normal, and a normal with length), a > 0 and DD > 0; otherwise g = +0.0.
 *   7. The closing emission is kept whole (m' = 1.0) under the conditions where the NEE rule keeps it.  Where the NEE rule drops it -- the previous
 *      vertex took a light sample and the emitter's primitive is sampled light l' (its first index in the list) -- it is weighted instead:
 *      s' = the emitter record's normal, normalised as step 3 of the hemisphere rule; cl' = |dot3(s', D)|, D = the arriving ray's direction as doubles;
 *      t = the record's t as a double; x' = ((((g * cl') / (t*t)) * area_l') * TWO_INV_PI) * q_l', g = the previous vertex' lobe value;
 *      m' = x' / (1.0 + x'), or 1.0 if x' is +inf, or +0.0 if x' is NaN.  radiance.c = accum.c + (double)emit.c * m'.
 *      (With d = t * D the NEE weight's cp^3 cl / d2^3 equals g * cl' / t^2: x' is the same density ratio, at the point the scatter found.)
 *   8. Unchanged from the NEE rule: nl == 0 (the call IS rtmi_render_rays), the refusal of media, the RTMI_F32 scope (weights and g are doubles whatever
 *      the precision), the four counters, the invariance under chunks and workspace passes.
 * Errors: the NEE calls', in their order, with light_choice other than 0 or 1 (RTMI_E_ARG) reported directly behind the list's length (n_lights), before
 * n_groups == 0 succeeds and before the media and the list's entries are looked at.
 * rtmi_probe_paths_mis: rtmi_probe_paths_nee's sibling.  log (may be NULL): [n][max_seg][RTMI_MIS_REC] doubles per logged vertex: [0..23] the RTMI_NEE_REC
 *   values (with light_choice 0, l, d and w are rtmi_probe_paths_nee's bit for bit; [21..23] the contribution of step 5); [24] x, [25] m, [26] g (zeros
 *   unless the vertex takes a light sample); [27] x' on a closing vertex whose emission step 7 weighted, else 0.  out_weight (may be NULL): [n] doubles,
 *   m' of step 7 -- 1.0 for every path whose closing emission is kept whole or that emits nothing. */
#define RTMI_MIS_REC 28
/* host buffers; synchronous */
int rtmi_render_rays_mis(rtmi_scene *scene, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first,
                         const double *rays, const uint64_t *keys, uint64_t seed, uint32_t ctr0, int32_t depth,
                         int32_t n_lights, const int32_t *light_prims, int32_t light_choice,
                         double *state, double *out_mean, double *out_stderr, double *out_rays, uint64_t *out_counters);
/* every d_ pointer a device pointer (light_prims stays a host array); asynchronous on `stream` with rtmi_render_device's stream semantics */
int rtmi_render_rays_mis_device(rtmi_scene *scene, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first,
                                const void *d_rays, const void *d_keys, uint64_t seed, uint32_t ctr0, int32_t depth,
                                int32_t n_lights, const int32_t *light_prims, int32_t light_choice,
                                void *d_state, void *d_out_mean, void *d_out_stderr, void *d_out_rays, void *d_out_counters, void *stream);
int rtmi_probe_paths_mis(rtmi_scene *scene, int32_t precision, int32_t n, const double *rays, const uint64_t *keys, uint64_t ctr0, int32_t depth,
                         int32_t n_lights, const int32_t *light_prims, int32_t light_choice, double *out_rgb, uint64_t *out_nseg, double *out_weight,
                         double *log, int32_t max_seg, int32_t *out_nlog);

/* ---- light-sampled frames from the scene's camera: the path calls above with their rays built on the device ----
 * rtmi_render_rays / _nee / _mis over the frame rtmi_render traces: no ray and no key is uploaded, a lane builds its camera ray in registers.
 *   n_groups = nx * ny, g_first = s_first, group = s_count; the state (may be NULL) is [nx*ny][RTMI_RAYS_REC], rtmi_render_rays' record and contract: any
 *   split of the samples into consecutive chunks (s_first = the samples already folded) gives the bits of one call; without a state s_first only offsets
 *   the keys and every call folds its own s_count samples.
 * THE FRAME RULE, operation by operation in the call's precision R (core.clj:43-51 and 105, camera.clj:8-16 and 35-48: rtmi_render's start of a sample).
 *   Row r of the call (0 <= r < nx*ny*s_count) belongs to group g = r / s_count and is sample s = s_first + (r - g * s_count).
 *   1. The pixel: x = g % nx, y = g / nx, row 0 at the top: j = ny - 1 - y.
 *   2. The stream: K = rtmi_sample_key(seed, j * nx + x, s), at draw 0.
 *   3. u = ((R)(float)x + draw 0) / (R)nx, v = ((R)(float)j + draw 1) / (R)ny: uniforms of R, one IEEE addition and one IEEE division each.
 *   4. The camera's get-ray with (u, v), from the camera the scene holds on the device, read in stream order (after rtmi_scene_set_camera / _stream: the
 *      new view).  RTMI_CAM_PINHOLE draws nothing more and the time is 0.  RTMI_CAM_THINLENS runs the unit-disk rejection loop (two draws per round, until
 *      x*x + y*y < 1; it runs with aperture 0 too) and then draws the time: the path starts at draw 2 + 2 * rounds + 1, a different one per sample.
 *   5. The attenuation is (1, 1, 1), the depth is the call's, and the path goes on in the SAME stream behind the camera's last draw.
 *   These are the operations of rtmi_render's samples: the path of row r is the path rtmi_render(nx, ny, ns > s, depth, seed, precision) traces for sample
 *   s of pixel (x, y), segment by segment.
 * estimator 0: the plain path of rtmi_render_rays (n_lights, light_prims and light_choice are not looked at); every scene rtmi_render_rays accepts, media
 *   included.  out_linear, out_stderr and the segment counter are rtmi_render's and rtmi_render_progressive's for (nx, ny, s_first + s_count, depth, seed,
 *   precision), bit for bit (with a state, or s_first = 0).
 * estimator 1: THE NEE RULE on those paths (light_choice is not looked at).  estimator 2: THE MIS RULE with light_choice.  Both with K of step 2 as the
 *   path's key; no light to sample: estimator 0 with the two shadow-ray counters zero.  They refuse a ConstantMedium and keep the rules' RTMI_F32 scope.
 *   out_linear: [ny][nx][3] the fold's mean (rtmi_render_rays' out_mean); out_stderr: [ny][nx]; out_rgb8 (may be NULL): [ny][nx][3], the frame's
 *   quantiser of out_linear, bit-equal to rtmi_denoise with zero passes; out_rays (may be NULL): [nx*ny*s_count][3], the radiance per row -- the call is
 *   then one pass; out_camera (may be NULL): [nx*ny*s_count][8] doubles per row: origin, direction, time and the stream position behind step 4, each
 *   widened from R; out_counters (may be NULL): FOUR values {segments, rays, shadow rays built, shadow rays occluded}.
 * Errors, in this order: nx, ny or s_count <= 0, s_first or depth < 0: RTMI_E_ARG; nx * ny * s_count > 2^31 - 64: RTMI_E_ARG; s_first + s_count
 * overflows int32: RTMI_E_ARG; out_linear or out_stderr NULL: RTMI_E_ARG; estimator outside 0..2: RTMI_E_ARG; then rtmi_render_rays' own from the scene
 * handle on (RTMI_E_STATE, the precision, RTMI_F32 with mixed kinds, Perlin, images); for estimators 1 and 2 the NEE / MIS calls' behind them (n_lights,
 * light_choice for estimator 2, the ConstantMedium, the list's entries); a host state whose counts are not s_first: RTMI_E_STATE.  A failed call
 * launches nothing.  Option "workspace_bytes" may split the call into passes of whole pixels: no bit changes.  The call touches neither the context's
 * progressive or adaptive frame nor the scene's revision; RTMI_FLAG_TIMING covers its passes as rtmi_render_rays'. */
/* host buffers; synchronous */
int rtmi_render_lit(rtmi_scene *scene, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                    int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice,
                    double *state, double *out_linear, uint8_t *out_rgb8, double *out_stderr, double *out_rays, double *out_camera,
                    uint64_t *out_counters);
/* every d_ pointer a device pointer (light_prims stays a host array); asynchronous on `stream` with rtmi_render_device's stream semantics */
int rtmi_render_lit_device(rtmi_scene *scene, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                           int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice,
                           void *d_state, void *d_out_linear, void *d_out_rgb8, void *d_out_stderr, void *d_out_rays, void *d_out_camera,
                           void *d_out_counters, void *stream);

/* ---- light-sampled paths and frames through participating media: the NEE and MIS rules on scenes that hold a ConstantMedium ----
 * The calls above refuse a ConstantMedium; these take it.  The reference's medium is itself a stochastic test: hit? scatters a ray whose chord in the
 * boundary has length L with probability 1 - exp(-density * L).  The same hit? run on a shadow ray with a draw of its own lets the ray through with
 * probability exactly exp(-density * L), the transmittance: the unoccluded flag is an unbiased estimate of it, no exp is evaluated, and the arithmetic
 * stays + - * / sqrt plus the medium's own log.  A medium the reference asks twice per ray is asked twice per shadow ray.  In the MIS ratio both
 * strategies carry the same transmittance, which cancels: x = w * q stays the density ratio.
 * THE VOLUME RULE, operation by operation as its siblings.  Where nothing is said the NEE rule (estimator 1) and the MIS rule (estimator 2) hold unchanged.
 * K = the path's key, j = the vertex' segment index, INV_4PI = 0x1.45f306dc9c883p-4.
 *   1. Vertices: a light sample is taken at every vertex where a RTMI_MAT_LAMBERTIAN or a RTMI_MAT_ISOTROPIC scatter happens (the depth left is > 0),
 *      and nowhere else.
 *   2. Light and point: the pick (stream rtmi_sample_key(K, j, 1)) and the point on the light (stream rtmi_sample_key(K, j, 0)) are unchanged, and so
 *      are d, d2, sd, cl, the far-side rule and the ray (p, d, time) with the t-range (0.001, 1 - 0.001); the time is the scattered ray's (at an
 *      Isotropic vertex the reference sets it to the hit's t, shader.clj:136, and every later vertex of the path inherits it).  At a Lambertian vertex
 *      everything is the NEE rule's.  At an Isotropic vertex the record's normal is not read (the reference's medium record carries an arbitrary one):
 *      the vertex is valid when p is finite; a ray is built when d2 > 0, cl > 0 and the far-side rule allows it; cp is not formed; p is the scatter point.
 *   3. The weight at an Isotropic vertex -- the reference scatters a medium hit uniformly over the sphere, density 1 / 4 pi:
 *      w = ((cl / (d2 * sqrt(d2))) * area) * INV_4PI.
 *   4. The shadow ray's stream is keyed rtmi_sample_key(K, j, 2) and starts at draw 0: the search is rtmi_query_occluded's on that ray with that key and
 *      ctr0 = 0.  The media are asked first, in the scene's call order; a medium that hits occludes the ray; a shadow ray that starts inside a medium is
 *      clipped as a path ray is.  The contributions are the siblings': NEE T * ((Le * w) * nl); MIS x = w * q_l, m = x / (1 + x), T * (Le * m).
 *   5. The MIS lobe value at an Isotropic vertex: DD = dot3(D, D); g = 0.125 / (DD * sqrt(DD)) if p is finite and DD > 0, else +0.0.  Step 7 of the MIS
 *      rule is unchanged and reads this g.  (With d = t * D, d2 = t*t * DD and cl = t * cl' for the unit normal: the weight of step 3 at the point the
 *      scatter found is cl' / (t*t * DD * sqrt(DD)) * area * INV_4PI = g * cl' / (t*t) * area * TWO_INV_PI with g = (INV_4PI / TWO_INV_PI) / (DD * sqrt(DD));
 *      INV_4PI / TWO_INV_PI = 1/8, exact -- both constants are the same significand.)
 *   6. The closing emission (NEE step 6, MIS step 7): "the previous vertex took a light sample" includes the Isotropic vertices.
 *   7. Scope.  Media mode RTMI_MEDIA_DESCENT only (every scene function of scene.clj); a scene in RTMI_MEDIA_HITLIST or the narrowed form returns
 *      RTMI_E_UNSUPPORTED and launches nothing (those worlds need the path kernels' media-sequence instantiations, which this family does not have).
 *      On a scene without media every output is the NEE or MIS sibling's bit for bit: no medium ever reads the new stream.  The RTMI_F32 scope is the
 *      siblings'.
 * rtmi_render_rays_vol*: rtmi_render_rays_mis' arguments with estimator (1 = the NEE rule, light_choice is not looked at; 2 = the MIS rule) in front of
 *   n_lights; the same state record, the same four counters, the same invariance under chunks and workspace passes.
 * rtmi_probe_paths_vol: rtmi_probe_paths_mis' arguments with estimator.  log: [n][max_seg][RTMI_VOL_REC]: [0..27] the RTMI_MIS_REC values (estimator 1:
 *   [21..23] the NEE contribution, [24..27] zeros); [28] = 1.0 where the light-sampled vertex is an Isotropic scatter.  out_weight: m'; for estimator 1,
 *   0.0 where the closing emission is dropped and 1.0 otherwise.
 * rtmi_render_lit_vol*: rtmi_render_lit's arguments, estimator 1 or 2 only; the same frame rule, state, out_camera, out_rays, 8-bit frame and counters.
 * Errors, in this order: the sibling's own, in its order, up to and including the list's length (n_lights); estimator outside {1, 2}: RTMI_E_ARG;
 * light_choice outside {0, 1} with estimator 2: RTMI_E_ARG; (n_groups == 0 succeeds here); media present and the mode not RTMI_MEDIA_DESCENT:
 * RTMI_E_UNSUPPORTED; the list's entries.  A failed call launches nothing and writes nothing. */
#define RTMI_VOL_REC 29
/* host buffers; synchronous */
int rtmi_render_rays_vol(rtmi_scene *scene, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first,
                         const double *rays, const uint64_t *keys, uint64_t seed, uint32_t ctr0, int32_t depth,
                         int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice,
                         double *state, double *out_mean, double *out_stderr, double *out_rays, uint64_t *out_counters);
/* every d_ pointer a device pointer (light_prims stays a host array); asynchronous on `stream` with rtmi_render_device's stream semantics */
int rtmi_render_rays_vol_device(rtmi_scene *scene, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first,
                                const void *d_rays, const void *d_keys, uint64_t seed, uint32_t ctr0, int32_t depth,
                                int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice,
                                void *d_state, void *d_out_mean, void *d_out_stderr, void *d_out_rays, void *d_out_counters, void *stream);
int rtmi_probe_paths_vol(rtmi_scene *scene, int32_t precision, int32_t n, const double *rays, const uint64_t *keys, uint64_t ctr0, int32_t depth,
                         int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice, double *out_rgb, uint64_t *out_nseg,
                         double *out_weight, double *log, int32_t max_seg, int32_t *out_nlog);
/* host buffers; synchronous */
int rtmi_render_lit_vol(rtmi_scene *scene, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                        int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice,
                        double *state, double *out_linear, uint8_t *out_rgb8, double *out_stderr, double *out_rays, double *out_camera,
                        uint64_t *out_counters);
/* every d_ pointer a device pointer (light_prims stays a host array); asynchronous on `stream` with rtmi_render_device's stream semantics */
int rtmi_render_lit_vol_device(rtmi_scene *scene, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                               int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice,
                               void *d_state, void *d_out_linear, void *d_out_rgb8, void *d_out_stderr, void *d_out_rays, void *d_out_camera,
                               void *d_out_counters, void *stream);

/* ---- light-sampled frames over a caller's list of 8x8 tiles: the primitive of an adaptive frame whose state the caller holds ----
 * rtmi_render_lit_tiles*: rtmi_render_lit's arguments, then volume, n_tiles and tiles in front of the state.  volume 0: rtmi_render_lit's rules, estimators
 *   0..2; volume 1: rtmi_render_lit_vol's, estimators 1..2.  tiles: n_tiles int32 -- a host array in the host form, a device array in the device form --
 *   of tile indices in rtmi_adaptive_active_tiles' numbering: tile t is row-major over T = ceil(nx/8) x ceil(ny/8) tiles, its local pixel l = row * 8 +
 *   column is pixel (x, y) = ((t % ceil(nx/8)) * 8 + l % 8, (t / ceil(nx/8)) * 8 + l / 8), row 0 at the top.  The call adds samples
 *   [s_first, s_first + s_count) to the pixels of the listed tiles and to nothing else.
 * THE TILE ORDER.  Row r of the call (0 <= r < n_tiles * 64 * s_count) is sample s = s_first + r % s_count of local pixel l = (r / s_count) % 64 of tile
 *   tiles[r / (64 * s_count)].  From that (x, y, s) on everything is THE FRAME RULE's steps 1 - 5 unchanged: j = ny - 1 - y, the key
 *   rtmi_sample_key(seed, j * nx + x, s), the jitter, the lens, the stream.  A row whose pixel lies outside the image (x >= nx or y >= ny: a partial tile's)
 *   builds no ray, traces nothing and counts nothing.
 *   state, out_linear, out_rgb8 and out_stderr keep the whole frame's layouts -- [nx*ny][RTMI_RAYS_REC], [ny][nx][3], [ny][nx][3], [ny][nx] -- and are
 *   in/out: the elements of the listed tiles' pixels inside the image are written with the fold's values (the state's records read first when s_first > 0,
 *   the 8-bit values quantised from the means just written), and every other element is neither written nor read by the device (the host form stages the
 *   whole planes both ways: those elements come back with the bits they went up with).  out_rays and out_camera (each may be NULL) are
 *   [n_tiles*64*s_count][3] and [...][8] in THE TILE ORDER, the rows of pixels outside the image +0.0; with out_rays the call is one pass.
 *   out_counters (may be NULL): rtmi_render_lit's four values for this call alone; rays = the listed pixels inside the image * s_count.
 *   For every listed pixel and every estimator the mean, the 8-bit value, the standard error and the state record are bit-identical to rtmi_render_lit
 *   (rtmi_render_lit_vol) of the whole frame with the same s_first, s_count and state; with all T tiles listed in ascending order every output and counter
 *   of the frame call is reproduced (out_rays and out_camera row by row through THE TILE ORDER).  Under estimator 0 the segment counter over a run of
 *   calls is rtmi_render_adaptive's over the same tiles and samples.  Option "workspace_bytes" may split the call into passes of whole tiles: no bit changes.
 * Errors, in this order: rtmi_render_lit's argument checks up to and including the estimator's range, the ray limit taken on n_tiles * 64 * s_count (and
 * nx * ny <= 2^31 - 64); volume outside {0, 1}: RTMI_E_ARG; n_tiles < 0, or tiles NULL with n_tiles > 0: RTMI_E_ARG; host form only: an entry outside
 * [0, T) or a list that is not strictly ascending: RTMI_E_ARG; then the sibling's checks from the scene handle on (with volume 1 the volume rule's: the
 * estimator in {1, 2}, the media mode) and its light checks; host form with a state and s_first > 0: a listed pixel inside the image whose count is not
 * s_first: RTMI_E_STATE.  n_tiles == 0 succeeds behind the argument checks and launches nothing.  A failed call launches nothing and writes nothing.
 * The device form cannot read its list back: there an entry outside [0, T) holds no pixel -- its rows build no ray and nothing of it is written, in the trace
 * kernel and in the fold alike, out_rays and out_camera included -- and duplicates and order are the caller's contract (a duplicated tile is folded twice,
 * in no defined order).  The call touches neither the context's progressive or adaptive frame nor the scene's revision. */
/* host buffers; synchronous */
int rtmi_render_lit_tiles(rtmi_scene *scene, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                          int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice,
                          int32_t volume, int32_t n_tiles, const int32_t *tiles,
                          double *state, double *out_linear, uint8_t *out_rgb8, double *out_stderr, double *out_rays, double *out_camera,
                          uint64_t *out_counters);
/* every d_ pointer a device pointer, d_tiles among them (light_prims stays a host array); asynchronous on `stream` with rtmi_render_device's stream semantics */
int rtmi_render_lit_tiles_device(rtmi_scene *scene, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                                 int32_t estimator, int32_t n_lights, const int32_t *light_prims, int32_t light_choice,
                                 int32_t volume, int32_t n_tiles, const void *d_tiles,
                                 void *d_state, void *d_out_linear, void *d_out_rgb8, void *d_out_stderr, void *d_out_rays, void *d_out_camera,
                                 void *d_out_counters, void *stream);

/* ---- light-sampled paths whose every lamp proposes a point: importance choice among the lights, one shadow ray per vertex ----
 * The NEE and MIS calls choose their light without looking at the vertex (uniformly, or by power).  In a room with many lamps a point is lit by the one or
 * two next to it, and a blind pick spends most shadow rays on lamps far away or facing the other way.  Here every listed light (at most
 * RTMI_DIRECT_MAX_LIGHTS) proposes one point at every vertex, each proposal is weighed by what it would contribute if it were visible, and a one-pass
 * weighted reservoir keeps one: the shadow ray goes where the light is.  These are new entries beside the MIS calls; the MIS siblings' arguments without
 * light_choice.
 * THE PROPOSAL RULE, operation by operation as its siblings: every product, sum, difference and quotient is one IEEE double operation in the order written,
 * only + - * / sqrt occur.  Where nothing else is said THE MIS RULE holds; K, j, nl, T and rtmi_sample_key are as defined there.
 *   1. Vertices: light samples are taken at the NEE rule's vertices (its step 1).  The path's own stream, rays, hits, scatters and segment count stay
 *      rtmi_render_rays' bit for bit.
 *   2. Candidates: every listed light l = 0 .. nl - 1 proposes one point, in list order: the NEE rule's steps 3 and 4 (point, d, d2, cp, cl, the far-side
 *      rule, the "no ray" conditions, w) with the stream keyed rtmi_sample_key(K, j, 4*l) at draw 0 -- light 0 uses the MIS rule's own stream and no light
 *      lands on streams 1 or 2.  x_l = w_l (every light proposes: the pick's inverse probability q is 1.0); m_l = x_l / (1.0 + x_l), or 1.0 if x_l is +inf.
 *      lum_l = (Le.r + Le.g) + Le.b, computed on the host and travelling with the light table; w^_l = lum_l * m_l.  A candidate is LIVE if it built a ray
 *      and w^_l > 0 and w^_l < +inf (a NaN fails).
 *   3. The choice, a one-pass weighted reservoir: S starts at +0.0; for each live candidate in list order S = S + w^_l; the first live candidate is taken;
 *      a later one replaces the chosen candidate if u_l * S < w^_l, u_l = the FP64 uniform of draw l of the stream keyed rtmi_sample_key(K, j, 1).
 *      A vertex with no live candidate builds no ray.
 *   4. The ray is the chosen candidate's; the any-hit search runs with the t-range (0.001, 1 - 0.001), as in the NEE rule.
 *   5. The contribution: if the search finds nothing, r = S / w^_sel and accum.c = accum.c + (double)T.c * ((Le_sel.c * m_sel) * r) per channel.
 *   6. The lobe value g: the MIS rule's step 6, unchanged.
 *   7. The closing emission: the MIS rule's step 7 with q_l' = 1.0 for every light.  A light whose lum_l is not > 0 can never be chosen: for this step it
 *      does not count as a sampled light and its emission is kept whole (as the power pick treats omega = 0; decided on the host).
 *   8. Unchanged from the MIS rule: nl == 0 (the call IS rtmi_render_rays), a ConstantMedium (RTMI_E_UNSUPPORTED), the RTMI_F32 scope (candidates, weights
 *      and g are doubles whatever the precision), the four counters ([2] counts the chosen candidates), the invariance under chunks and workspace passes.
 *   Over the choice the expectation of step 5 is the sum over l of Le_l * m_l * V_l: the light strategy "one point on every light", whose density on light l
 *   is 1 / area_l; m_l depends on the proposed point alone, and step 7 gives the scatter the complementary share at the point it found.  Every
 *   contribution is at most T.c * (Le_sel.c / lum_sel) * (the sum of lum_k over the lights).  With one light of positive emission r is exactly 1.0 and every
 *   output equals the MIS rule's under light_choice 0 -- except at a vertex whose ray the MIS rule builds with a share m of +0.0 (w underflowed): that
 *   candidate is not live here, so the vertex builds no ray: state 3, zeros for l, d, w, x, m in the log, and counter [2] does not count it.  Its
 *   contribution is +0.0 under either rule, so the radiance is the same.
 * rtmi_probe_paths_ris: rtmi_probe_paths_mis without light_choice.  log (may be NULL): [n][max_seg][RTMI_RIS_REC] doubles per logged vertex: [0..27] the
 *   RTMI_MIS_REC values for the chosen candidate ([12] the state, 3 = a light-sampled vertex with no live candidate: l, d, w, x, m are then zeros);
 *   [28] S, [29] w^_sel, [30] r, [31] the number of live candidates (zeros where the vertex takes no light sample).
 * rtmi_render_rays_ris*: rtmi_render_rays_mis* without light_choice.
 * rtmi_render_lit_ris*: the frame of the scene's own camera: rtmi_render_lit_tiles*' arguments without estimator, light_choice and volume.  tiles NULL:
 *   the whole frame -- n_tiles is not read, the rows, out_rays, out_camera and every layout are rtmi_render_lit's (the SRC_CAMERA kernels).  tiles not
 *   NULL: THE TILE ORDER, the in/out whole-frame buffers and every other word of rtmi_render_lit_tiles*.  THE FRAME RULE, the RTMI_RAYS_REC state and the
 *   counters are the siblings'.
 * Errors: the MIS calls' (rtmi_render_lit_tiles*' for the frame with a list, rtmi_render_lit*'s without), in their order, less the checks of the removed
 * arguments.  A failed call launches nothing and writes nothing.  Out of scope: media, more than RTMI_DIRECT_MAX_LIGHTS lights, proposals at metal or
 * glass, reuse of candidates between pixels or frames. */
#define RTMI_RIS_REC 32
/* host buffers; synchronous */
int rtmi_render_rays_ris(rtmi_scene *scene, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first,
                         const double *rays, const uint64_t *keys, uint64_t seed, uint32_t ctr0, int32_t depth,
                         int32_t n_lights, const int32_t *light_prims,
                         double *state, double *out_mean, double *out_stderr, double *out_rays, uint64_t *out_counters);
/* every d_ pointer a device pointer (light_prims stays a host array); asynchronous on `stream` with rtmi_render_device's stream semantics */
int rtmi_render_rays_ris_device(rtmi_scene *scene, int32_t precision, int32_t n_groups, int32_t group, int32_t g_first,
                                const void *d_rays, const void *d_keys, uint64_t seed, uint32_t ctr0, int32_t depth,
                                int32_t n_lights, const int32_t *light_prims,
                                void *d_state, void *d_out_mean, void *d_out_stderr, void *d_out_rays, void *d_out_counters, void *stream);
int rtmi_probe_paths_ris(rtmi_scene *scene, int32_t precision, int32_t n, const double *rays, const uint64_t *keys, uint64_t ctr0, int32_t depth,
                         int32_t n_lights, const int32_t *light_prims, double *out_rgb, uint64_t *out_nseg, double *out_weight,
                         double *log, int32_t max_seg, int32_t *out_nlog);
/* host buffers; synchronous */
int rtmi_render_lit_ris(rtmi_scene *scene, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                        int32_t n_lights, const int32_t *light_prims, int32_t n_tiles, const int32_t *tiles,
                        double *state, double *out_linear, uint8_t *out_rgb8, double *out_stderr, double *out_rays, double *out_camera,
                        uint64_t *out_counters);
/* every d_ pointer a device pointer, d_tiles among them (light_prims stays a host array); asynchronous on `stream` with rtmi_render_device's stream semantics */
int rtmi_render_lit_ris_device(rtmi_scene *scene, int32_t precision, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count, int32_t depth, uint64_t seed,
                               int32_t n_lights, const int32_t *light_prims, int32_t n_tiles, const void *d_tiles,
                               void *d_state, void *d_out_linear, void *d_out_rgb8, void *d_out_stderr, void *d_out_rays, void *d_out_camera,
                               void *d_out_counters, void *stream);

/* rtmi_tiles_retire*: the stateless rtmi_adaptive_retire -- the decision of that call on a list the caller holds; no frame of the context is read or changed.
 *   noise: [ny][nx] doubles of the whole frame, row 0 at the top: rtmi_render_lit_tiles' out_stderr or rtmi_denoise's filtered error as it is.  A listed tile
 *   SURVIVES if any of its pixels inside the image fails noise <= eps, the comparison written exactly so: NaN and +inf fail, -inf passes (a pixel of one
 *   sample, whose standard error is +inf, keeps its tile).  The survivors go to tiles_out in the order of tiles_in, *out_count (a host int32 in both forms) is
 *   their number; tiles_out holds n_tiles entries, may be tiles_in itself, and its entries from *out_count on keep what they held.
 * Errors, all reported before the handle is examined: nx or ny <= 0, noise NULL, eps negative, NaN or infinite: RTMI_E_ARG; n_tiles < 0, tiles_in or
 * tiles_out NULL with n_tiles > 0, out_count NULL: RTMI_E_ARG; host form only: an entry outside [0, T): RTMI_E_ARG.  Then the handle: RTMI_E_STATE.
 * n_tiles == 0 sets *out_count = 0 and launches nothing.  The device form synchronises `stream` once, as rtmi_adaptive_retire_device does, and queues the
 * copy of the survivors into d_tiles_out behind it, in stream order; there an entry outside [0, T) reads no element of the map outside the image. */
int rtmi_tiles_retire(rtmi_ctx *ctx, int32_t nx, int32_t ny, const double *noise, double eps, int32_t n_tiles, const int32_t *tiles_in, int32_t *tiles_out,
                      int32_t *out_count);
int rtmi_tiles_retire_device(rtmi_ctx *ctx, int32_t nx, int32_t ny, const void *d_noise, double eps, int32_t n_tiles, const void *d_tiles_in,
                             void *d_tiles_out, int32_t *out_count, void *stream);

/* After the gather: d_gathered[r][k][64][3] (r < world, k < tiles_per_rank, rank r's k-th tile is global
 * tile r + k*world) -> dense row-major frame (doubles, may be NULL) + 8-bit frame (may be NULL). */
int rtmi_assemble_device(rtmi_ctx *ctx, int32_t nx, int32_t ny, int32_t world, int32_t tiles_per_rank,
                         const void *d_gathered, void *d_out_linear, void *d_out_rgb8, void *stream);

/* ---- progressive and adaptive frames on dealt tiles: the per-device primitive of a frame refined on several GPUs ----
 * rtmi_render_adaptive_tiles_device is to rtmi_render_progressive* / rtmi_render_adaptive* what rtmi_render_tiles_device is to rtmi_render: the
 * context's one progressive frame covers the DEALT tiles tile_first, tile_first + tile_stride, ... (global row-major tile indices over
 * ceil(nx/8) x ceil(ny/8); rtmi_local_tiles of them; local tile k is global tile tile_first + k * tile_stride), its region is the whole image,
 * and the call writes tile records instead of a dense frame.
 *   The dealing is part of the frame's key.  The entries above are the dealing (0, 1): a whole-frame (0, 1) frame may be continued by either
 *   family; a continuation with another dealing is RTMI_E_STATE and rtmi_last_error names both dealings.
 *   retire = 0: rtmi_render_progressive's semantics on those tiles -- samples [s_first, s_first + s_count) to every tile, no tile retires, eps is
 *               not read; refused with RTMI_E_STATE (frame untouched) if a tile of the frame has retired.
 *   retire = 1: rtmi_render_adaptive's two steps with eps (trace the active tiles, then retire those whose pixels all pass se <= eps at k >= 2),
 *               under the same argument rules.
 *   d_tiles_rec[k][64][RTMI_PROG_REC] doubles, may be NULL: local tile k, pixel l = row * 8 + column of the tile.  With n_t the samples the tile holds:
 *               values 0-2 the mean over samples [0, n_t), computed with the resolve's own expression sums * (R(1) / R(n_t)) in the precision R of
 *               the frame and widened to double; value 3 the standard error exactly as rtmi_render_adaptive's out_stderr defines it (+inf for
 *               n_t = 1); value 4 n_t as a double.  Pixels outside the image hold five zeros.
 *   d_out_counters, may be NULL: {ray segments traced into this frame so far, pixels of the dealt tiles that lie inside the image}.
 * Like rtmi_render_adaptive_device the call synchronises the stream once, at its end, for either value of retire.
 * rtmi_progressive_samples, rtmi_adaptive_status, rtmi_adaptive_active_tiles (global tile indices, ascending), rtmi_adaptive_retire* (the map is
 * still the WHOLE frame's [ny][nx]; only the frame's own active tiles are read) and rtmi_progressive_release work on a dealt frame as they do on
 * a whole one.  A rank dealt no tile (tile_first beyond the last tile) holds an empty frame that still counts its samples.
 * Errors: tile_first < 0, tile_stride <= 0, s_first < 0, s_count <= 0, retire outside {0, 1}, with retire = 1 an eps that is negative, NaN or
 * infinite: RTMI_E_ARG, reported before the handle is examined; the others are the progressive calls'.  A failure before anything is launched
 * leaves the frame as it was; a failure after a launch drops it. */
#define RTMI_PROG_REC 5   /* doubles per pixel of a progressive tile record: mean r, g, b, stderr, samples */
int rtmi_render_adaptive_tiles_device(rtmi_scene *scene, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count,
                                      int32_t retire, double eps, int32_t depth, uint64_t seed, int32_t precision,
                                      int32_t tile_first, int32_t tile_stride, void *d_tiles_rec, void *d_out_counters, void *stream);
/* After the gather of such records: d_gathered_rec[r][k][64][RTMI_PROG_REC] (r < world, k < tiles_per_rank as for rtmi_assemble_device, rank r's
 * k-th tile is global tile r + k*world; slots past the last tile are ignored) -> the dense frame.  Outputs, each of which may be NULL:
 * linear [ny][nx][3] doubles, rgb8 (assemble_device's quantiser on the mean: the double one, whatever the frame's precision), stderr [ny][nx]
 * doubles, samples [ny][nx] int32.  Asynchronous on `stream` (rtmi_render_device's stream semantics). */
int rtmi_assemble_progressive_device(rtmi_ctx *ctx, int32_t nx, int32_t ny, int32_t world, int32_t tiles_per_rank,
                                     const void *d_gathered_rec, void *d_out_linear, void *d_out_rgb8, void *d_out_stderr, void *d_out_samples, void *stream);

/* ---- one host process, several GPUs ---------------------------------------------------------------
 * The reference's host is ONE JVM whose render loop fans out over a thread pool (cp/upmap, core.clj:100-108); the same
 * single process reaches the 8 GPUs of a node through these entries: one context per device (rtmi_init), the scene
 * replicated onto each (rtmi_scene_clone; it is tiny), the framebuffer's 8x8 tiles dealt round-robin (replica r renders
 * global tiles r, r+n, ...: the reference's tiled-coords chunks, core.clj:59-71), ONE gather over xGMI to replica 0's
 * device -- ncclGather on a communicator the library creates with ncclCommInitAll and owns (librccl is opened on first
 * use; a single-GPU host never loads it) -- and replica 0 un-tiles / quantises.  Pixels are independent and the stream key is
 * the global pixel index: the image is bit-identical to the single-device render.
 * Replicas that share a device (to rehearse the control flow on a one-GPU host) are gathered by device copies instead, and so
 * is a host on which librccl cannot be opened or initialised, or whose gather failed once (one line on stderr).
 * RTMI_MULTI_GATHER=rccl: RCCL or an error, never a substitution -- and a ONE-replica call then goes through the whole RCCL path too
 * (dlopen, ncclCommInitAll of one rank, grouped in-place ncclGather): that is how the path is executed on a one-GPU host (status:
 * the one-rank path runs in the GPU test suite; a communicator over several devices has not run yet -- no multi-GPU host so far).
 * RTMI_MULTI_GATHER=copy forces the copies.  rtmi_last_gather_path says which one ran.
 * On an error after the first replica's launch every replica stream touched so far is synchronised before the call returns. */
/* Replicates `scene` onto `ctx` (another device): the library copied the caller's arrays at creation. */
int rtmi_scene_clone(rtmi_scene *scene, rtmi_ctx *ctx, rtmi_scene **out_scene);
/* Replaces core.clj:100-108 on n devices.  scenes[r] = replica r (each on its own context).  Host buffers as rtmi_render
 * (whole frame); out_counters = {total-rays summed over the replicas, total-pixels}. */
int rtmi_render_multi(int32_t n, rtmi_scene *const *scenes, int32_t nx, int32_t ny, int32_t ns, int32_t depth, uint64_t seed,
                      int32_t precision, double *out_linear, uint8_t *out_rgb8, uint64_t *out_counters);
/* The same, asynchronous, outputs resident on replica 0's device (ordered on replica 0's context stream; every replica
 * renders on its own context stream). */
int rtmi_render_multi_device(int32_t n, rtmi_scene *const *scenes, int32_t nx, int32_t ny, int32_t ns, int32_t depth, uint64_t seed,
                             int32_t precision, void *d_out_linear, void *d_out_rgb8, void *d_out_counters);
/* One progressive / adaptive frame refined on n devices: every replica r calls rtmi_render_adaptive_tiles_device's work with the dealing (r, n)
 * on its own context stream (the launches of the replicas overlap), ONE gather -- the paths and RTMI_MULTI_GATHER values above: same-device
 * copies, peer copies, the grouped ncclGather with its count scaled to the larger record; n = 1 launches none -- moves the records to replica 0's
 * device, and replica 0 assembles.  Outputs as rtmi_render_adaptive's for the whole frame, each may be NULL; out_counters = {ray segments
 * summed over the replicas, pixels of the frame}.  retire and eps as for rtmi_render_adaptive_tiles_device.
 * For every n, either gather path, F64 and F32, sphere-only and mixed-kind scenes, any sequence of chunk sizes and any "workspace_bytes" split,
 * out_linear, out_rgb8, out_stderr, out_samples and out_counters[0] are BIT-IDENTICAL to what one context returns from rtmi_render_adaptive for
 * the whole frame after the same calls (with retire = 0: from rtmi_render_progressive), and the union of the replicas' active lists
 * (rtmi_adaptive_active_tiles on each context) is that context's active list: pixels are independent, every draw is keyed by (seed, global pixel,
 * sample), and a tile retires on its own pixels alone.
 * The argument checks and the continuation checks of ALL replicas run before the first launch: a mismatch on any replica (RTMI_E_STATE, the text
 * names the replica) leaves every frame as it was.  A failure after a launch drops the frame on EVERY replica -- a later s_first > 0 is refused
 * on the whole set -- and every stream touched so far is synchronised before the call returns.  Both forms return with every replica's stream
 * synchronised (the host mirrors every replica's active list), so rtmi_adaptive_status / rtmi_adaptive_retire* may follow on each context. */
int rtmi_render_multi_adaptive(int32_t n, rtmi_scene *const *scenes, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count,
                               int32_t retire, double eps, int32_t depth, uint64_t seed, int32_t precision,
                               double *out_linear, uint8_t *out_rgb8, double *out_stderr, int32_t *out_samples, uint64_t *out_counters);
/* The same, outputs resident on replica 0's device. */
int rtmi_render_multi_adaptive_device(int32_t n, rtmi_scene *const *scenes, int32_t nx, int32_t ny, int32_t s_first, int32_t s_count,
                                      int32_t retire, double eps, int32_t depth, uint64_t seed, int32_t precision,
                                      void *d_out_linear, void *d_out_rgb8, void *d_out_stderr, void *d_out_samples, void *d_out_counters);
/* ---- light-sampled frames on several GPUs: THE DEALT LIT FRAME ----
 * One light-sampled frame -- uniform or adaptive, under the plain estimator, the NEE rule, the MIS rule (with or without the volume rule) or the
 * proposal rule -- refined on n replicas of a scene.  What rtmi_render_multi_adaptive is to rtmi_render_adaptive these entries are to
 * rtmi_render_lit_tiles / rtmi_render_lit_ris with a list and rtmi_tiles_retire: the sample path and the decision are those calls' own, keyed by
 * (seed, global pixel, sample) and taken per tile from that tile's pixels alone, so nothing in them knows who owns a tile.
 *   THE RECORD.  rtmi_lit_tiles_records_device packs dealt tiles out of a replica's WHOLE-FRAME buffers into the record of the dealt progressive
 *   frames above: d_out_rec[n_slots][64][RTMI_PROG_REC] doubles, slot k = global tile tile_first + k * tile_stride, local pixel l = row * 8 + column
 *   (THE TILE ORDER's numbering).  Values 0-2 are the pixel's three doubles of d_linear [ny][nx][3] and value 3 its double of d_stderr [ny][nx], copied
 *   as they are (rtmi_render_lit_tiles' out_linear and out_stderr); value 4 is word [9], the sample count, of the pixel's record in d_state
 *   [nx * ny][RTMI_RAYS_REC].  A pixel outside the image holds five zeros, and so does every pixel of a slot whose tile is at or past
 *   T = ceil(nx/8) * ceil(ny/8): those slots are the padding of a gathered record, so a gather never moves uninitialised memory.  No tile list is
 *   read.  rtmi_assemble_progressive_device assembles the gathered records unchanged; its quantiser and rtmi_render_lit_tiles' are one function
 *   (sqrt, x 255.99, min, truncation, NaN -> 0 on the double mean), so the 8-bit frame is the single context's too.
 *   Errors, all reported before the handle is examined: nx or ny <= 0 or more than 2^30 pixels, tile_first < 0, tile_stride <= 0, n_slots < 0 or
 *   > 2^24, a NULL buffer with n_slots > 0: RTMI_E_ARG.  Then the handle: RTMI_E_STATE.  n_slots == 0 launches nothing.  Asynchronous on `stream`. */
int rtmi_lit_tiles_records_device(rtmi_ctx *ctx, int32_t nx, int32_t ny, int32_t tile_first, int32_t tile_stride, int32_t n_slots, const void *d_state,
                                  const void *d_linear, const void *d_stderr, void *d_out_rec, void *stream);
/*   THE FRAME is an object the library owns, named by a 64-bit handle that is never 0 (a JNA host holds a long).  rtmi_multi_lit_create takes
 *   n = 1 .. RTMI_MULTI_LIT_MAX replicas of one scene, each on its own context, as rtmi_render_multi takes them (replaces the caller's buffers of
 *   rtmi_render_lit_tiles_device, per device).  Per replica the frame holds the whole-frame state (RTMI_RAYS_REC doubles = 80 bytes per pixel), the
 *   linear and stderr planes, the replica's tile list and its record; on replica 0's device the gathered records.  Whole-frame buffers on every
 *   replica cost n times the memory a compact layout would -- 166 MB of state per device at 1920 x 1080, 232 MB with the planes -- because the
 *   sample path indexes its state by the global pixel; a compact layout would mean editing those kernels.
 *   THE DEALING is round-robin: replica r owns tiles r, r + n, ... and starts with all of them listed, ascending.  A replica that owns no tile
 *   (n > T) is legal and launches no trace.  Every replica's record holds per = ceil(T / n) slots.
 *   rtmi_multi_lit_destroy frees the buffers (after every replica's stream is idle); destroy the frame before its scenes. */
#define RTMI_MULTI_LIT_MAX 8
int rtmi_multi_lit_create(int32_t n, rtmi_scene *const *scenes, int32_t nx, int32_t ny, uint64_t *out_frame);
int rtmi_multi_lit_destroy(uint64_t frame);
/*   THE CALL ORDER.  rtmi_multi_lit_render adds samples [k, k + s_count) to every listed tile, k being the frame's own count (the samples its active
 *   tiles hold; 0 after create and reset): on every replica, on its own context stream, rtmi_render_lit_tiles_device's work on the replica's list with
 *   `estimator` 0, 1, 2 and `volume` 0 or 1 -- estimator 3 is the proposal rule, rtmi_render_lit_ris_device's work with a list, which has no volume
 *   form -- then the record of its dealt tiles and the call's four counters behind them; all replicas are enqueued before any is waited for.  ONE
 *   gather -- rtmi_render_multi's paths and RTMI_MULTI_GATHER values: same-device copies, peer copies, the grouped ncclGather; rtmi_last_gather_path
 *   and rtmi_last_gather_ms on replica 0's context report it; n = 1 moves nothing -- brings per * 320 + 4 eight-byte words per replica to replica 0's
 *   device, which assembles the frame and sums the counters (replaces rtmi_render_lit_tiles / rtmi_render_lit_ris on one context).
 *   Outputs, each may be NULL, host arrays in the first form and buffers on replica 0's device in the second: linear [ny][nx][3] doubles, rgb8
 *   [ny][nx][3], stderr [ny][nx] doubles, samples [ny][nx] int32, counters[4] = rtmi_render_lit_tiles' four of THIS call summed over the replicas.
 *   For every n, either gather path, every estimator, F64 and F32, any sequence of chunk sizes and any "workspace_bytes" split they are BIT-IDENTICAL
 *   to what one context holds after the same rtmi_render_lit_tiles / rtmi_tiles_retire calls on one list.  Both forms return with every replica's
 *   stream synchronised.
 *   rtmi_multi_lit_retire: every replica runs rtmi_tiles_retire_device on its own list (replaces rtmi_tiles_retire on one list).  noise NULL: each
 *   replica tests its own stderr plane, which is valid on exactly its own tiles -- all the decision reads.  Otherwise noise is a whole-frame map
 *   [ny][nx], on the host (first form) or on replica 0's device and complete on its context stream (second form) -- the denoiser's filtered error --
 *   and is sent to every replica first.  *out_count = the tiles still listed, summed over the replicas.
 *   rtmi_multi_lit_status: *out_k = k, *out_active = the listed tiles of all replicas (either may be NULL).  rtmi_multi_lit_active_tiles: the
 *   replicas' lists merged in ascending order into out_tiles[capacity]; *out_count is their number, and a capacity below it is RTMI_E_ARG with
 *   *out_count set.  rtmi_multi_lit_reset: k = 0 and every tile listed again; no buffer is freed.
 *   THE KEY.  The first render after create or reset fixes precision, depth, seed, estimator, volume, light_choice (where the estimator reads it), the
 *   light list and the revisions of the replicas' scenes.  A later render under another key is RTMI_E_STATE and rtmi_last_error gives both keys.  A
 *   camera, material or geometry edit of a scene changes its revision: a frame is not continued across an edit, it is reset.
 *   Errors of a render, in this order: frame 0, s_count <= 0, depth < 0, estimator outside 0..3, volume outside {0, 1}, estimator 3 with volume 1, an
 *   unknown precision: RTMI_E_ARG, before the handle is examined; a handle that names no frame: RTMI_E_STATE; n_lights outside the sibling's range, a
 *   light_choice the MIS rule does not know: RTMI_E_ARG; the key: RTMI_E_STATE; then, replica by replica, the sibling's own checks in its order (the
 *   scene's tables, an ineligible listed light: RTMI_E_ARG, the media mode: RTMI_E_UNSUPPORTED; the text names the replica) and the gather policy.
 *   Every check of every replica runs before the first launch: a refusal leaves the frame exactly as it was.  A failure after a launch resets the
 *   frame on every replica once every touched stream is idle.  rtmi_multi_lit_retire: frame 0, an eps that is negative, NaN or infinite, out_count
 *   NULL: RTMI_E_ARG; a bad handle or a frame without samples: RTMI_E_STATE. */
int rtmi_multi_lit_render(uint64_t frame, int32_t precision, int32_t s_count, int32_t depth, uint64_t seed, int32_t estimator, int32_t n_lights,
                          const int32_t *light_prims, int32_t light_choice, int32_t volume, double *out_linear, uint8_t *out_rgb8, double *out_stderr,
                          int32_t *out_samples, uint64_t *out_counters);
int rtmi_multi_lit_render_device(uint64_t frame, int32_t precision, int32_t s_count, int32_t depth, uint64_t seed, int32_t estimator, int32_t n_lights,
                                 const int32_t *light_prims, int32_t light_choice, int32_t volume, void *d_out_linear, void *d_out_rgb8, void *d_out_stderr,
                                 void *d_out_samples, void *d_out_counters);
int rtmi_multi_lit_retire(uint64_t frame, const double *noise, double eps, int32_t *out_count);
int rtmi_multi_lit_retire_device(uint64_t frame, const void *d_noise, double eps, int32_t *out_count);
int rtmi_multi_lit_status(uint64_t frame, int32_t *out_k, int32_t *out_active);
int rtmi_multi_lit_active_tiles(uint64_t frame, int32_t capacity, int32_t *out_tiles, int32_t *out_count);
int rtmi_multi_lit_reset(uint64_t frame);
/* How the last rtmi_render_multi* on replica 0's context moved the replicas' records to replica 0's device. */
enum { RTMI_GATHER_NONE = 0,        /* one replica: nothing to move */
       RTMI_GATHER_SAME_DEVICE = 1, /* replicas share replica 0's device (rehearsal on a one-GPU host): device-to-device copies */
       RTMI_GATHER_PEER_COPY = 2,   /* distinct devices, hipMemcpyPeerAsync (RTMI_MULTI_GATHER=copy, or RCCL unusable on this host) */
       RTMI_GATHER_RCCL = 3 };      /* ONE grouped ncclGather on the library's communicator set */
int rtmi_last_gather_path(rtmi_ctx *ctx0, int32_t *path);
/* Can the RCCL library `soname` be opened and does it export the entry points the in-library gather binds (ncclCommInitAll,
 * ncclCommDestroy, ncclGroupStart, ncclGroupEnd, ncclGather, ncclGetErrorString)?  soname = NULL: the names the gather itself tries
 * ("librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", or $RTMI_RCCL_LIB).  Touches no device.  RTMI_E_DEVICE + the loader's
 * message when not. */
int rtmi_rccl_probe(const char *soname);
/* *idle = 1 when nothing is pending on the context's own stream (hipStreamQuery). */
int rtmi_stream_idle(rtmi_ctx *ctx, int32_t *idle);
/* Sample passes (trace-kernel launches) the context's most recent render took: the per-sample colour buffer is sized by option
 * "workspace_bytes", by the HBM that is free when it has to grow (at most 80 % of it) and, if the allocation still fails, by halving. */
int rtmi_last_passes(rtmi_ctx *ctx, int32_t *passes);
/* Reals per sample record of the context's most recent render that traced: 4 = it deferred (option "defer_emitters"), 3 = it did not; 0 before any. */
int rtmi_last_record_reals(rtmi_ctx *ctx, int32_t *reals);
/* RTMI_ACCEL_* the context's most recent render actually ran: option "accel" as set, except that a small mixed-kind scene (option
 * "flat_below") is scanned even when the tree was asked for.  RTMI_E_STATE before the first render. */
int rtmi_last_accel(rtmi_ctx *ctx, int32_t *accel);
/* Milliseconds between the end of replica 0's own render and the end of the gather of the last rtmi_render_multi* on
 * replica 0's context (HIP events on its stream): the transfer plus the wait for the slowest replica. */
int rtmi_last_gather_ms(rtmi_ctx *ctx0, double *ms);

/* The reference's third counter, metrics.clj:10 `aabb.intersection.total` (incremented once per AABB.hit?, hitable.clj:39),
 * for the device's own tree: *out_aabb_tests = AABB slab tests, *out_prim_tests = exact primitive tests (leaves + the
 * primitives kept out of the tree) of the context's most recent render.  Needs option "count_traversal" = 1 before that
 * render (a separate kernel instantiation: the default kernel does not pay for the counting); synchronises on the render's
 * stream.  The numbers depend on the tree the library built, not on the reference's random-axis tree. */
int rtmi_last_traversal_counters(rtmi_ctx *ctx, uint64_t *out_aabb_tests, uint64_t *out_prim_tests);

/* Total milliseconds of the trace-kernel launches of every render on this context since the previous call
 * (HIP events recorded on the launch stream around each launch; needs RTMI_FLAG_TIMING; synchronises on the
 * last event; at most 8192 launches are kept).  *launches = kernel launches covered.  Resets the window. */
int rtmi_last_trace_ms(rtmi_ctx *ctx, double *ms, int32_t *launches);
/* The in-order sample reductions (reduce_kernel, core.clj:52-53) of the measurement window the last rtmi_last_trace_ms call closed:
 * sum of their durations (from each trace kernel's end event to the event after its reduction) and their number. */
int rtmi_last_reduce_ms(rtmi_ctx *ctx, double *ms, int32_t *launches);

/* ---- probes: the same device functions the render kernel runs, one protocol call at a time ---- */
/* Hitable.hit? of the world for n rays {o.xyz, d.xyz, time}; out[n][11] = hit?, prim, t, p.xyz, normal.xyz, u, v */
int rtmi_probe_hit(rtmi_scene *scene, int32_t precision, int32_t n, const double *rays, double t_min, double t_max, double *out);
/* `color` (core.clj:17-41) of n explicit rays with their own stream keys; log (may be NULL):
 * [n][max_seg][RTMI_SEG_REC]; out_nlog[n] segments logged. */
int rtmi_probe_paths(rtmi_scene *scene, int32_t precision, int32_t n, const double *rays, const uint64_t *keys, uint64_t ctr0,
                     int32_t depth, double *out_rgb, uint64_t *out_nseg, double *log, int32_t max_seg, int32_t *out_nlog);
/* Camera.get-ray for n (u,v) pairs; out[n][8] = o.xyz, d.xyz, time, draws consumed */
int rtmi_probe_camera(rtmi_scene *scene, int32_t precision, int32_t n, const double *uv, const uint64_t *keys, double *out);
/* Texture.sample of texture `tex` for n {u, v, p.xyz}; out[n][3] */
int rtmi_probe_texture(rtmi_scene *scene, int32_t precision, int32_t tex, int32_t n, const double *uvp, double *out);
/* Shader.scatter of material `mat` for n rays and hit records {p.xyz, normal.xyz, u, v};
 * out[n][9] = scattered?, dir.xyz, attenuation.rgb, time, draws consumed */
int rtmi_probe_scatter(rtmi_scene *scene, int32_t precision, int32_t mat, int32_t n, const double *rays, const double *hits,
                       const uint64_t *keys, double *out);
/* The counter stream: out_bits[k] = 64 raw bits, out_real[k] = the uniform in [0,1) for draw index d0+k of `key` */
int rtmi_probe_rng(rtmi_ctx *ctx, int32_t precision, uint64_t key, uint64_t d0, int32_t n, uint64_t *out_bits, double *out_real);
/* sample key of (seed, pixel index j*nx+i, sample) -- pure host function, no device needed */
uint64_t rtmi_sample_key(uint64_t seed, uint64_t pixel, uint64_t sample);
/* correctly-rounded device arithmetic check: out[k] = {a/b, sqrt(|a|), a*b+c unfused} */
int rtmi_probe_arith(rtmi_ctx *ctx, int32_t n, const double *abc, double *out);
/* the path's own FP64 helpers, one thread per triple (a, b, c):  out[n_slots k + j], j < n_slots <= RTMI_PROBE_MATH_SLOTS =
 * { 0 sqrt(a) (fast path for finite arguments >= 2^-767, libm otherwise), 1 atan2(a, b), 2 asin(a), 3, 4 u and v of get-sphere-uv for the unit normal
 * (a, b, c) (hitable.clj:128-139), 5 a / b through the per-ray reciprocal of the sphere roots (t-min / t-max decide with b whether the lane takes
 * it), 6 a / (2 pi) by the constant-divisor form, 7 1.0 if the lane took the reciprocal path else 0.0, 8 the traversal's float bound of a closest hit at
 * t = c: a float >= c within two ulps (FLT_MAX beyond the float range), 9 log(a) as ConstantMedium's free-flight distance evaluates it for a draw a in
 * [0, 1), 10 a / b through the refined reciprocal of a SIGNED divisor (a rectangle's t = (k - o) / d), 11 1.0 if slot 10 took the reciprocal path }.
 * The caller's buffer holds n * n_slots doubles: the slot count is an argument so that a host built against an older header is never overrun.
 * rtmi_probe_math is the entry as first published: the first EIGHT slots (library version 203 wrote nine; from 204 on it is eight again). */
#define RTMI_PROBE_MATH_SLOTS 12
int rtmi_probe_math2(rtmi_ctx *ctx, int32_t n, const double *abc, double tmin, double tmax, int32_t n_slots, double *out);
int rtmi_probe_math(rtmi_ctx *ctx, int32_t n, const double *abc, double tmin, double tmax, double *out);

/* test hook, host arithmetic only (no device): the IEEE half (bits) at or beyond x in the given direction -- what the tree's half-plane node records are
 * rounded with (up != 0: the smallest half >= x, else the largest half <= x; +-inf beyond the half range) */
int rtmi_test_build_tree(int32_t n, const double *geom, const double *cam, int32_t threads, uint64_t *out_hash, int32_t *out_info, double *out_ms);
/* ^ test hook, host code only: the device's tree and entry grid over n spheres (geom[n][4] = cx cy cz r) exactly as rtmi_scene_create builds them -- on the
 * library's team of build threads, or with threads = 1 on the calling thread alone; out_hash = FNV-1a of the node array and the grid's root codes (the same
 * for any thread count), out_info[4] = node records, depth, grid cells per side, big primitives; out_ms = the build's wall time */
int rtmi_test_camera_fixed(int32_t cam_kind, const double *cam);
/* ^ test hook, host arithmetic only (no device): bit 0 = every ray of the camera cam[24] starts at cam[0..2] bit for bit (the stash carries no origins), bit 1 = a
 * thin lens whose offset changes no bit of a ray's direction either (the wave-wide refill only counts the lens disk's draws) */
int rtmi_test_half_outward(double x, int32_t up); /* x: a float value (host scalars are doubles at this boundary) */
/* test hook, host code only (no device): the eleven material tables of rtmi_scene_create_ex's arrays, packed as rtmi_scene_set_materials* packs an edit
 * (through_creation = 0: only prim_kind, prim_mat and the material and texture tables are read, the other arrays may be NULL) or as creation packs them
 * (through_creation = 1: after creation's checks, as part of the whole scene).  out_hash = FNV-1a of the tables (equal for both: one packer),
 * out_facts[3] = the materials' share of has_ext, uses_perlin, max_image.  The errors are those of the path taken. */
int rtmi_test_pack_materials(int32_t n_prims, const int32_t *prim_kind, const double *prim_geom, const int32_t *prim_mat,
                             int32_t n_mats, const int32_t *mat_kind, const int32_t *mat_tex, const double *mat_param,
                             int32_t n_tex, const int32_t *tex_kind, const double *tex_param, const int32_t *tex_child,
                             int32_t cam_kind, const double *cam, const int32_t *prim_flip, const int32_t *prim_xform,
                             int32_t n_xforms, const int32_t *xform_kind, const double *xform_param, int32_t through_creation,
                             uint64_t *out_hash, int32_t *out_facts);
/* test hook, host code only (no device): the geometry tables of rtmi_scene_create_ex's arrays -- stat_geom, stat4_d, stat4_f, exact12, cull20, leaf_rec,
 * ext_xf, mov_geom, media_fast_of, every primitive's bounded flag and world box -- as creation packs them (through_creation = 1) or as
 * rtmi_scene_set_geometry packs an edit (0), both after creation's checks.  out_hash = FNV-1a of them (equal for both: one packer). */
int rtmi_test_pack_geometry(int32_t n_prims, const int32_t *prim_kind, const double *prim_geom, const int32_t *prim_mat,
                            int32_t n_mats, const int32_t *mat_kind, const int32_t *mat_tex, const double *mat_param,
                            int32_t n_tex, const int32_t *tex_kind, const double *tex_param, const int32_t *tex_child,
                            int32_t cam_kind, const double *cam, const int32_t *prim_flip, const int32_t *prim_xform,
                            int32_t n_xforms, const int32_t *xform_kind, const double *xform_param, int32_t through_creation, uint64_t *out_hash);
/* test hook, host code only (no device): the trees of geometry 0 as creation builds them (every surface one grey Lambertian, every medium Isotropic), then steps 1 .. n_steps - 1 as
 * rtmi_scene_set_geometry (mode 0) applies them -- the same fit and displacement rules, a rebuild where a step does not fit -- with the refit done by the
 * host's reference of refit_kernel's rule.  geoms[n_steps][n_prims][RTMI_PRIM_STRIDE], xforms[n_steps][n_xforms][3] (NULL with n_xforms = 0).  The state
 * after the last step: out_nodes (if *out_bytes <= capacity) the node array, out_info[10] = node16, bvh_root, grid_tall, grid cells per side, n_big,
 * displaced, rebuilt by the last step, node records, refit launches, steps that rebuilt since step 0; out_big[16] (may be NULL) the big list; out_cells
 * (may be NULL) up to cells_capacity of the grid's 4 G G root codes; out_leaf_box (may be NULL) [n_world][6] floats lo.xyz hi.xyz, the leaf boxes of the last
 * in-place step ((+inf, -inf): not in the trees). */
int rtmi_test_refit(int32_t n_prims, const int32_t *prim_kind, const int32_t *prim_flip, const int32_t *prim_xform, int32_t n_xforms, const int32_t *xform_kind,
                    int32_t cam_kind, const double *cam, int32_t n_steps, const double *geoms, const double *xforms,
                    void *out_nodes, int64_t capacity, int64_t *out_bytes, int32_t *out_info, int32_t *out_big,
                    int32_t *out_cells, int64_t cells_capacity, void *out_leaf_box);
int rtmi_test_refit_half(double x, int32_t up); /* rtmi_test_half_outward by the integer form the refit uses on the device */
/* test hook: the scene's node array as it lies in HBM, after the work queued on the context's stream; *out_bytes = its size, copied if <= capacity */
int rtmi_test_scene_nodes(rtmi_scene *scene, void *buf, int64_t capacity, int64_t *out_bytes);
/* test hook, host code only (no device): where the host forms' staging puts n planes of elem_bytes[i] * counts[i] bytes each, by the code that lays out
 * every host form's device buffers (present[i] = 0: an optional array the caller left out).  out_offsets[i] = the plane's first byte (UINT64_MAX for an
 * absent plane), *out_total = the bytes the staging buffer needs */
int rtmi_test_stage_layout(int32_t n, const uint64_t *elem_bytes, const uint64_t *counts, const int32_t *present, uint64_t *out_offsets, uint64_t *out_total);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_H */
