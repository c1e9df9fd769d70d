/*
 * zrt.h — C ABI of the MI355X path tracer (libzrt.so).
 *
 * This is the drop-in boundary for the reference's per-pixel Monte-Carlo
 * sampling loop.  The reference seam is
 *
 *     pub fn render(allocator: *Allocator, random: *Random,
 *                   camera: Camera, surfaces: ArrayList(Surface),
 *                   render_params: RenderParams) !*Image
 *                                              (src/raytrace.zig:136-138)
 *
 * A Zig caller flattens `ArrayList(Surface)` (src/surface.zig:12-16), the
 * `*const Material` pointers (src/material.zig:16-52), the `Texture` values
 * (src/texture.zig:7-28) and the `*Image` pointers they reference into the flat
 * arrays of `zrt_scene`, keeping the reference list order, and calls
 * `zrt_render`.  See INTEGRATION.md for the `@cImport` adapter.
 *
 * Conventions (all from the reference):
 *   - f32 everywhere (src/base.zig:2).
 *   - Framebuffer: width*height RGB f32, row-major, row 0 = bottom of the image
 *     (src/raytrace.zig:164-182, src/image.zig:74-78).
 *   - Texture images: same layout, already flipped and scaled by 1/255 as
 *     src/png_image.zig:76-89 produces them.
 *   - Camera: the four vectors `Camera.init` computes (src/camera.zig:17-35);
 *     `zrt_camera_init` restates `Camera.init` on the host (tan stays on host).
 *
 * Errors: every entry point returns ZRT_OK (0) or a negative ZRT_E_* code and
 * leaves a message in a thread-local buffer read by `zrt_last_error()`.  This
 * maps 1:1 onto a Zig error union (`!*Image`).  No C++ exception crosses the ABI.
 *
 * Ownership: the library copies every input during the call and keeps no
 * pointer into caller memory after it returns.  `out_rgb` is caller-allocated.
 * Device memory is owned by the library (zrt_render) or by a zrt_ctx handle.
 * The library is not reentrant on one zrt_ctx; distinct contexts may be used
 * from distinct threads.
 */
#ifndef ZRT_H
#define ZRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: zrt_stats gained sampling_loop (its size changed) and zrt_build_id was added;
 * a client built against version 1 must not pass its smaller zrt_stats. */
#define ZRT_ABI_VERSION 2

/* ---- status codes ------------------------------------------------------- */
enum {
  ZRT_OK = 0,
  ZRT_E_INVALID = -1,     /* bad argument (e.g. unknown kind, index out of range) */
  ZRT_E_NOMEM = -2,       /* host or device allocation failed (Zig: OutOfMemory) */
  ZRT_E_HIP = -3,         /* HIP runtime error */
  ZRT_E_UNSUPPORTED = -4, /* valid for the reference, not provided by this path */
  ZRT_E_NODEVICE = -5,    /* no usable MI355X (gfx950) device */
  ZRT_E_IO = -6,          /* asset file missing / unreadable */
  ZRT_E_PARSE = -7        /* OBJ parse error (obj_reader.zig ParseError) */
};

/* ---- scene description (flattened ArrayList(Surface)) ------------------- */
enum { ZRT_PRIM_SPHERE = 0, ZRT_PRIM_TRIANGLE = 1 };          /* surface.zig:12-16 */
enum { ZRT_MAT_LAMBERTIAN = 0, ZRT_MAT_METAL = 1, ZRT_MAT_DIELECTRIC = 2 }; /* material.zig:27-29 */
enum { ZRT_TEX_COLOR = 0, ZRT_TEX_IMAGE = 1 };                /* texture.zig:7-9 */

typedef struct zrt_vec3 { float x, y, z; } zrt_vec3;          /* vector.zig:22-25 */

/* Camera.{origin, lower_left_corner, horizontal, vertical} (camera.zig:11-15). */
typedef struct zrt_camera {
  zrt_vec3 origin;
  zrt_vec3 lower_left_corner;
  zrt_vec3 horizontal;
  zrt_vec3 vertical;
} zrt_camera;

/* One element of ArrayList(Surface).  kind selects the union member:
 *   SPHERE:   center, radius            (Sphere.init, sphere.zig:24-29)
 *   TRIANGLE: a, b, c (vertex order kept: Triangle.init, triangle.zig:32-44)
 * `material` indexes zrt_scene.materials (the deduplicated *const Material). */
typedef struct zrt_prim {
  uint32_t kind;
  uint32_t material;
  zrt_vec3 center;
  float radius;
  zrt_vec3 a, b, c;
} zrt_prim;

/* Material union (material.zig:16-52).  `texture` indexes zrt_scene.textures
 * and is used by LAMBERTIAN and METAL; `index_of_refraction` by DIELECTRIC. */
typedef struct zrt_material {
  uint32_t kind;
  uint32_t texture;
  float index_of_refraction;
} zrt_material;

/* Texture union (texture.zig:7-28): COLOR uses `color`; IMAGE uses `image`
 * (index into zrt_scene.images), `u_offset`, `v_offset` (Texture.initImage
 * passes 0.19, 0.1: texture.zig:14-16). */
typedef struct zrt_texture {
  uint32_t kind;
  uint32_t image;
  zrt_vec3 color;
  float u_offset;
  float v_offset;
} zrt_texture;

/* Image (image.zig:74-78): width*height RGB f32, row 0 = bottom. */
typedef struct zrt_image {
  uint32_t width;
  uint32_t height;
  const float* pixels;
} zrt_image;

/* Degenerate geometry is accepted and traced as the reference traces it: zero-area
 * and zero-size primitives, duplicates, leaves whose box is flat on an axis (which the
 * reference BVH never opens), coordinates up to FLT_MAX, +-inf and NaN vertices.
 * One thing is refused, by every entry point that takes a scene, with
 * ZRT_E_UNSUPPORTED and a message naming the primitive: a primitive whose bounding
 * box (sphere.zig:24-29, triangle.zig:33) has a NaN midpoint on some axis - a NaN
 * bound (a NaN sphere centre or radius) or a box from -inf to +inf (an infinite
 * radius).  The reference sorts midpoints with `<` (bvh.zig:85-120), which does not
 * order a NaN: its tree is then an accident of the sort algorithm, and no two
 * implementations of "the reference's BVH" agree on it.  Nothing finite is refused. */
typedef struct zrt_scene {
  const zrt_prim* prims;         /* reference list order (scenes.zig append order) */
  uint32_t n_prims;
  uint32_t n_materials;
  const zrt_material* materials;
  const zrt_texture* textures;
  uint32_t n_textures;
  uint32_t n_images;
  const zrt_image* images;
} zrt_scene;

/* ---- render parameters (RenderParams, raytrace.zig:102-108) ------------- */
enum {
  ZRT_RNG_COUNTER = 0,          /* per-(pixel,sample) stream; the GPU mode */
  ZRT_RNG_REFERENCE_STREAM = 1  /* one sequential stream as the reference; CPU oracle only */
};
enum { ZRT_PRNG_XOROSHIRO128 = 0, ZRT_PRNG_XOSHIRO256 = 1 };
enum {
  /* FAST: a 4-wide SAH tree built over the reference BVH's leaves culls with
   * the narrowed slab test; every leaf reached is put through the reference's
   * own slab test; equal-t ties go to the earlier leaf in the reference's DFS
   * order.  Same answers as REFERENCE. */
  ZRT_TRAVERSAL_FAST = 0,
  ZRT_TRAVERSAL_REFERENCE = 1,  /* left-first DFS with exactly bvh.zig:187-205's tests */
  ZRT_TRAVERSAL_BINARY = 2      /* near-first over the reference BVH itself, narrowed + loose tests */
};

typedef struct zrt_params {
  uint32_t width;                    /* RenderParams.width (u16 in the reference) */
  uint32_t height;                   /* RenderParams.height */
  uint32_t samples_per_pixel;        /* RenderParams.samples_per_pixel */
  uint32_t max_depth;                /* RenderParams.max_depth */
  uint32_t bounded_volume_hierarchy; /* RenderParams.bounded_volume_hierarchy (BVH iff also n>10) */
  uint32_t rng_mode;                 /* ZRT_RNG_* */
  uint32_t prng;                     /* ZRT_PRNG_* (DefaultPrng variant) */
  uint32_t traversal;                /* ZRT_TRAVERSAL_* */
  uint64_t seed;                     /* DefaultPrng.init(seed); the scenes use 42 */
  uint32_t rank;                     /* image-tile partition: this rank ... */
  uint32_t world_size;               /* ... of world_size (1 = whole frame) */
  uint32_t device;                   /* HIP device ordinal */
  /* COUNTER mode: a pixel's samples are summed in chunks of sample_chunk
   * consecutive samples (each chunk sequentially, as raytrace.zig:177 does),
   * and the chunk sums are then added in chunk order.  0 selects 32
   * (ZRT_DEFAULT_SAMPLE_CHUNK).  With sample_chunk >= samples_per_pixel this is
   * the reference's single sequential sum.  A chunk is the kernel's unit of
   * work: shorter units end a launch sooner. */
  uint32_t sample_chunk;
  uint32_t flags;                    /* ZRT_FLAG_* */
  uint32_t reserved;
} zrt_params;

/* flags: ZRT_FLAG_STATS launches the diagnostic flavour of the kernel that also
 * counts BVH node visits, primitive tests, shaded hits and texel fetches
 * (zrt_stats).  Images are identical; the default flavour counts only the
 * Progress counters (raytrace.zig:20-34). */
enum { ZRT_FLAG_STATS = 1u, ZRT_FLAG_NO_SCHEDULE = 2u, ZRT_FLAG_SCANLINES = 4u, ZRT_FLAG_GUARD = 8u };
enum { ZRT_DEFAULT_SAMPLE_CHUNK = 32u };
/* Scheduling (FAST traversal, spp >= 128, unless ZRT_FLAG_NO_SCHEDULE): a probe
 * launch renders 1 sample per pixel of every tile (results discarded) and
 * records each tile's cost; the tiles are radix-sorted by descending cost on
 * the device and the render launch hands out units costliest first, so no long
 * unit starts at the end of the launch.  Images do not depend on it.
 * A context keeps the last probe's order: a later frame with the same camera
 * (compared bitwise), width, height, max_depth, rank, world_size, traversal, guard
 * flag and tile count - whatever its samples_per_pixel, seed or prng - skips the
 * probe and the sort, and reports schedule_ms = 0.  ZRT_ORDER_CACHE=0 in the
 * environment probes every frame (A/B).
 * All-sky tiles (the lockstep FAST loop, max_depth >= 1, no ZRT_FLAG_SCANLINES or
 * ZRT_FLAG_GUARD, a frame or a progressive pass): the tiles the host proves no
 * primary ray can hit anything in (zrt_debug_tile_classes) render in a kernel of
 * their own without traversal; the frame and the counters are the same bit for bit.
 * The classes are kept under the same key as the order; classifying counts into
 * schedule_ms of a launch that probes.  ZRT_SKY_TILES=0 turns the split off (A/B).
 * One-sphere tiles (the same launches, where the scene and the params also allow the
 * lean kernel - solid-colour Lambertian and metal materials, no ZRT_FLAG_SCANLINES;
 * with or without ZRT_FLAG_STATS): the tiles the host proves no primary ray can hit
 * anything in but one sphere whose leaf is a child of the wide tree's root render in
 * an instance of the lockstep kernel whose camera rays test that sphere alone instead
 * of walking the tree; every later ray of a path is traced as before, and the frame
 * and the counters are the same bit for bit (STATS counts such a ray as one ray and one
 * sphere test, no node visit).  Where a frame has such tiles for several spheres, those of
 * the sphere with the most are taken.  ZRT_SPHERE_TILES=0 leaves them general (A/B);
 * ZRT_SPHERE_TILES=2 sends their list through a launch of the unchanged render kernel (what
 * they cost there); either needs the all-sky split on. */

/* ZRT_FLAG_GUARD (FAST traversal): the grazing-triangle guard (DESIGN.md
 * section 3 "Triangles"): every box is widened by the reach of the rounded
 * triangle test (triangle.zig:48-70) for rays nearly parallel to a triangle,
 * whose accepted hits can lie outside their leaf's box.  zrt_trace always uses
 * it; a render uses it (in the path-pool loop) when this flag is set - the
 * reference's scenes render bit for bit the same frames without it, at a third
 * more speed on the teapot.  zrt_stats.guard reports the coefficient used. */

/* ZRT_FLAG_SCANLINES: the launch also counts the recursion-limit hits,
 * reflections and background hits of every frame row (the deltas that
 * printProgress prints after each scanline, raytrace.zig:37-50, 184), read
 * back with zrt_ctx_scanlines / zrt_multi_scanlines / zrt_render_progress.
 * Images and totals are unchanged; the counts are added per finished work
 * unit (a few atomics per 8x8 tile x sample chunk), so the flag costs little
 * but is off in the timed bench. */

/* Progress counters (raytrace.zig:20-34) + timings. */
typedef struct zrt_stats {
  uint64_t recursion_depth_hits;
  uint64_t reflections;
  uint64_t background_hits;
  uint64_t pixels_processed;
  uint64_t samples_processed;
  uint64_t rays_processed;
  uint64_t node_visits;   /* BVH nodes whose box was tested (diagnostic) */
  uint64_t prim_tests;    /* primitive intersection tests, triangles + spheres */
  uint64_t sphere_tests;  /* ... of which spheres */
  uint64_t shade_fetches; /* closest hits shaded (hit record + material reads) */
  uint64_t texel_fetches; /* image-texture lookups */
  uint64_t leaf_visits;   /* FAST traversal: reference leaf boxes tested (node_visits = wide nodes) */
  double preprocess_ms;   /* BVH build + flatten (raytrace.zig:150) */
  double upload_ms;
  double render_ms;       /* device time of the sampling loop: schedule probe + sort + render kernel */
  double gather_ms;
  uint32_t used_bvh;      /* preprocessSufraces decision (raytrace.zig:124-133) */
  uint32_t bvh_nodes;
  uint32_t bvh_max_depth; /* Tracking.max_depth (bvh.zig:23-30) */
  uint32_t n_gpus;
  uint32_t node_bytes;    /* bytes of one node record of the traversal used (32 or 128) */
  uint32_t wide_nodes;    /* FAST traversal: 4-wide nodes over the reference leaves */
  uint32_t texel_bytes;   /* bytes per texel on the device: 4 when every image is exact 8-bit
                             (c == k/255, png_image.zig:76-89), else 12 (f32 RGB); 0: no images */
  float schedule_ms;       /* probe + sort before the render launch (included in render_ms); 0 when the
                            * context's kept tile order was reused */
  uint64_t order_replays;  /* FAST: rays re-traced the reference's way for an order hazard (diagnostic) */
  /* REFERENCE traversal + ZRT_FLAG_STATS (diagnostic, DESIGN.md §3 "Exactness"):
   * over every primitive of every leaf the reference opens, the largest
   * max(E/t - 1, t/X - 1) of its hit t (t_max = inf) against the leaf box's
   * loose entry E and exit X - how far rounded hits lie outside their own
   * box - per primitive kind, and how many hits lie out by more than 2^-14. */
  float box_excess_max_triangle;
  float box_excess_max_sphere;
  uint64_t box_excess_hits;
  /* the sampling loop of the last launch: 0 surface list, 1
   * binary / 2 reference BVH traversal, FAST traversal: 3 lockstep, 4 wavefront,
   * 5 path pool; 6 surface list with per-lane work items */
  uint32_t sampling_loop;
  /* the grazing-triangle guard's coefficient of the launch (0: off; ZRT_FLAG_GUARD) */
  float guard;
} zrt_stats;

/* One frame row's share of the Progress counters (raytrace.zig:20-34): what
 * raytrace.zig:184's printProgress(y + 1, ...) reports for scanline y as
 * deltas (recursion limit, reflections, background hits) and as running sums
 * (pixels, samples, rays: add rows 0..y).  rays = samples + reflections -
 * recursion_depth_hits (every rayColor call with depth > 0, raytrace.zig:69). */
typedef struct zrt_scanline {
  uint64_t recursion_depth_hits;
  uint64_t reflections;
  uint64_t background_hits;
  uint64_t pixels;
  uint64_t samples;
  uint64_t rays;
} zrt_scanline;

/* ---- entry points -------------------------------------------------------- */

/* Replaces raytrace.render (raytrace.zig:136-203): render the whole frame on
 * one GPU (params->device).  out_rgb: width*height*3 f32, caller-allocated.
 * rng_mode must be ZRT_RNG_COUNTER.  stats may be NULL. */
int zrt_render(const zrt_scene* scene, const zrt_camera* camera,
               const zrt_params* params, float* out_rgb, zrt_stats* stats);

/* zrt_render that also returns the per-scanline counters of raytrace.zig:184
 * (scanlines: params->height entries, row 0 = bottom, as the reference's y). */
int zrt_render_progress(const zrt_scene* scene, const zrt_camera* camera,
                        const zrt_params* params, float* out_rgb, zrt_stats* stats,
                        zrt_scanline* scanlines);

/* raytrace.render (raytrace.zig:136-203) over several GPUs of one node, from one
 * host thread: the frame's 8x8 tiles are dealt round-robin
 * over devices[0..n_devices) (tile t -> rank t % n_devices), every GPU holds its
 * own copy of the scene and renders its tiles concurrently, and ONE RCCL gather
 * (ncclGather over xGMI, ncclCommInitAll communicators) collects them on
 * devices[0], where they are assembled and copied to out_rgb.  The image is
 * bit-identical to zrt_render's for any device list.  A device listed more
 * than once runs several ranks (tests on one GPU); RCCL takes one rank per
 * device, so such a list gathers with device-to-device copies instead.  RCCL
 * (librccl.so.1) is opened on first use.  params->rank / world_size / device
 * are ignored.  stats: counters summed over ranks, render_ms = the slowest
 * rank's, gather_ms = gather + assemble, n_gpus = distinct devices. */
int zrt_render_multi(const zrt_scene* scene, const zrt_camera* camera,
                     const zrt_params* params, const uint32_t* devices,
                     uint32_t n_devices, float* out_rgb, zrt_stats* stats);

/* zrt_render_multi split into a persistent multi-GPU context (a Zig host
 * rendering many frames of one scene): zrt_multi_create builds the BVH once,
 * uploads the scene to every device of the list and creates the RCCL
 * communicators once (one rank per distinct device, >= 2 devices; otherwise
 * the tiles move by device copies and RCCL is not loaded).
 * zrt_multi_render renders one frame as zrt_render_multi does (same image,
 * same stats); params->rank / world_size / device are ignored and
 * params->bounded_volume_hierarchy must imply the create-time BVH decision.
 * out_rgb may be NULL: the assembled frame then stays in devices[0]'s HBM
 * (a frame loop that times the GPUs, not the PCIe copy) and zrt_multi_frame
 * copies it out later. */
typedef struct zrt_multi zrt_multi;
int zrt_multi_create(const zrt_scene* scene, const zrt_params* params,
                     const uint32_t* devices, uint32_t n_devices, zrt_multi** out);
int zrt_multi_render(zrt_multi* multi, const zrt_camera* camera,
                     const zrt_params* params, float* out_rgb, zrt_stats* stats);
int zrt_multi_destroy(zrt_multi* multi);
/* The last zrt_multi_render's frame (n_floats = width * height * 3, row 0 =
 * bottom) copied from devices[0] to out_rgb. */
int zrt_multi_frame(zrt_multi* multi, float* out_rgb, uint64_t n_floats);
/* The last zrt_multi_render's render-kernel time of each rank in ms (HIP
 * events around its launch; n = n_devices of zrt_multi_create). */
int zrt_multi_rank_ms(zrt_multi* multi, double* kernel_ms, uint32_t n);
/* Per-scanline counters of the last zrt_multi_render made with
 * ZRT_FLAG_SCANLINES, summed over the ranks (height = params->height). */
int zrt_multi_scanlines(zrt_multi* multi, zrt_scanline* out, uint32_t height);

/* The closest-hit query of one rayColor step (raytrace.zig:71-81: the top-level
 * surfaces tested with t_min = 0.001 and a shrinking t_max; under BVH that is
 * BVHNode.hit, bvh.zig:187-205) for a batch of rays on params->device, through
 * the render loop's own traversal (params->traversal).  rays: n_rays x {origin
 * xyz, direction xyz}, directions normalised as Ray.init does (ray.zig:11-13).
 * out_t: the hit's t (+inf on a miss); out_prim: the index of the surface hit
 * in scene->prims (-1 on a miss).  One-shot like zrt_render. */
int zrt_trace(const zrt_scene* scene, const zrt_params* params, const float* rays,
              uint32_t n_rays, float* out_t, int32_t* out_prim);

/* Restates Camera.init (camera.zig:17-35).  look_from/look_at/vup: float[3]. */
int zrt_camera_init(const float look_from[3], const float look_at[3],
                    const float vup[3], float vfov_deg, float aspect_ratio,
                    zrt_camera* out);

/* Thread-local message for the last error on this thread ("" if none). */
const char* zrt_last_error(void);

/* ABI version (ZRT_ABI_VERSION) and build identity string. */
int zrt_abi_version(void);
const char* zrt_build_info(void);
/* What the kernels of this library were built from: sha1 of the device and
 * tree-layout sources + zrt.h (16 hex digits) - sha1 of the device compile
 * flags (8).  Performance-counter records are keyed by it (bench.py). */
const char* zrt_build_id(void);

/* ---- device-resident context (bench / multi-GPU) ------------------------ *
 * zrt_ctx_create does preprocessSufraces (BVH build, raytrace.zig:124-133),
 * flattens the scene and uploads it once to params->device.  zrt_ctx_render
 * then runs only the sampling loop, reading the resident scene and writing a
 * device buffer, so a timed region sees no host<->device traffic.           */
typedef struct zrt_ctx zrt_ctx;

int zrt_ctx_create(const zrt_scene* scene, const zrt_params* params, zrt_ctx** out);
int zrt_ctx_destroy(zrt_ctx* ctx);

/* Number of 8x8 tiles this (rank, world_size) owns; its tile buffer holds
 * n_tiles*64*3 floats.  Tiles are dealt round-robin: tile t -> rank t % world.
 * Tiles cover x in [0, height) (raytrace.zig:168's bound) by y in [0, height).
 * Host-only: ctx may be NULL. */
int zrt_ctx_tile_count(const zrt_ctx* ctx, const zrt_params* params, uint32_t* n_tiles);

/* Render this rank's tiles into dev_tiles (device pointer, tile-major,
 * n_tiles*64*3 f32) on `hip_stream` (a hipStream_t; NULL = the context's own
 * stream, a blocking stream, so work the caller later enqueues on the legacy
 * default stream waits for it).  Asynchronous: returns after enqueueing.
 * zrt_ctx_sync / zrt_ctx_stats / zrt_ctx_last_kernel_ms wait for the launch
 * (on whichever stream it ran) and return ZRT_E_UNSUPPORTED if the device
 * reported an error (a traversal stack overflow); such a launch also writes
 * NaN to every pixel of dev_tiles, and the next zrt_ctx_render_tiles on the
 * context returns the error if the launch has finished by then.
 * params->device must be the context's device, and params->
 * bounded_volume_hierarchy must imply the BVH decision the context was built
 * with (ZRT_E_INVALID otherwise). */
int zrt_ctx_render_tiles(zrt_ctx* ctx, const zrt_camera* camera,
                         const zrt_params* params, float* dev_tiles,
                         void* hip_stream);

/* This rank's per-scanline counters of the last launch, which must have been
 * made with ZRT_FLAG_SCANLINES (ZRT_E_INVALID otherwise); out: height entries
 * (rows of the frame; rows this rank owns no tiles of stay zero). Waits. */
int zrt_ctx_scanlines(zrt_ctx* ctx, zrt_scanline* out, uint32_t height);

/* Wait for the context's last launch; ZRT_OK, or ZRT_E_UNSUPPORTED when the
 * device reported an error during it (see zrt_ctx_render_tiles). */
int zrt_ctx_sync(zrt_ctx* ctx);

/* Scatter gathered tiles of all ranks (rank-major: rank r's n_tiles(r) tiles
 * follow rank r-1's) into the framebuffer layout of raytrace.zig:182.
 * dev_gathered / dev_frame are device pointers; runs on hip_stream. */
int zrt_ctx_assemble(zrt_ctx* ctx, const zrt_params* params,
                     const float* dev_gathered, float* dev_frame, void* hip_stream);

/* The same from the layout a gather of equal per-rank counts produces: rank r's
 * tiles start at tile r * stride_tiles (stride_tiles >= every rank's count;
 * the tiles past a rank's count are padding and are not read). */
int zrt_ctx_assemble_padded(zrt_ctx* ctx, const zrt_params* params,
                            const float* dev_gathered, uint32_t stride_tiles,
                            float* dev_frame, void* hip_stream);

/* Counters of the last zrt_ctx_render_tiles (waits for that launch). */
int zrt_ctx_stats(zrt_ctx* ctx, zrt_stats* out);

/* Raw device counter slots of the last launch (diagnostics; n <= 32):
 * [0..9] progress/traffic counters, [14] work counter, [15] error flag,
 * [16..20] per-section cycle sums of ZRT_PROFILE builds. */
int zrt_ctx_debug_counters(zrt_ctx* ctx, uint64_t* out, uint32_t n);

/* The last launch's schedule (diagnostics): per local tile, the probe's cost
 * (loop iterations its wave spent on ZRT_PROBE_SPP samples per pixel), and the tile order
 * the render launch used.  *n_tiles = 0 when the launch was not scheduled. */
int zrt_ctx_debug_schedule(zrt_ctx* ctx, uint32_t* costs, uint32_t* order, uint32_t cap, uint32_t* n_tiles);

/* ZRT_PROFILE builds only (diagnostics): {start, end} s_memrealtime stamps
 * (100 MHz) of every wave of the last render launch; *n_waves = 0 otherwise. */
int zrt_ctx_debug_wave_times(zrt_ctx* ctx, uint64_t* out, uint32_t cap, uint32_t* n_waves);

/* Duration in ms of the last zrt_ctx_render_tiles' kernel (HIP events on the
 * launch stream; synchronises). */
int zrt_ctx_last_kernel_ms(zrt_ctx* ctx, double* ms);

/* ---- progressive rendering: sample passes accumulated on a context --------- *
 * A sample's random stream is keyed by (pixel, sample index, seed) and not by
 * samples_per_pixel, and a pixel is the sequential sum of its chunk sums
 * (raytrace.zig:177) times 1 / samples_per_pixel (raytrace.zig:157, 182).  So a
 * frame can be rendered in passes of whole sample chunks, each added onto a
 * resident per-pixel sum: after every pass the resolved frame (sum x 1 / samples
 * done) equals, bit for bit, a full render with samples_per_pixel = samples
 * done, and the chunk sums a launch parks in memory are the pass's, not the
 * frame's.
 *
 * zrt_ctx_accum_begin starts a run: it fixes the camera and every param
 * (validated as zrt_ctx_render_tiles validates them; samples_per_pixel is the
 * run's cap, the planned total).  One run is live per context: a second begin
 * restarts it, and any zrt_ctx_render_tiles on the context ends it (the
 * scheduling probe's buffers belong to the context).
 *
 * zrt_ctx_accum_pass renders the next n_samples samples of every pixel through
 * zrt_ctx_render_tiles' launch path and kernels, adds them to the accumulator
 * and writes the resolved tiles (this rank's, as zrt_ctx_render_tiles lays them
 * out) to dev_tiles.  Asynchronous; every pass of a run goes to one stream (or
 * to streams the caller orders).  ZRT_E_INVALID: n_samples == 0, a pass past the
 * cap, a pass that does not start on a sample chunk boundary (a ragged pass is
 * allowed and is then the run's last, as the frame's ragged last chunk is), or
 * no live run.  The run schedules once, by the rule of ZRT_FLAG_NO_SCHEDULE with
 * the cap as samples_per_pixel: its first pass probes, later passes reuse the
 * tile order (their schedule_ms is 0).  After a pass zrt_ctx_stats,
 * zrt_ctx_scanlines report the run's counters so far - what a full render of
 * samples_done samples counts - with render_ms / schedule_ms summed over the
 * passes; zrt_ctx_last_kernel_ms is the last pass's.  A device error in a pass
 * is sticky for the run: NaN tiles from then on, ZRT_E_UNSUPPORTED from
 * zrt_ctx_sync / zrt_ctx_stats / zrt_ctx_accum_info and from later passes. */
typedef struct zrt_pass_info {
  uint32_t samples_done;    /* samples per pixel in the accumulator after the pass */
  uint32_t pass_samples;    /* of them, this pass */
  uint64_t changed_pixels;  /* this rank's pixels whose 8-bit PNG value changed in the pass */
  float    max_abs_change;  /* largest |new - previous| over this rank's channels (previous = 0 before pass 1) */
  float    render_ms;       /* this pass: probe (if any) + render kernel, as zrt_stats.render_ms */
  float    schedule_ms;     /* this pass's probe + sort; 0 when the run's cached order was reused */
  uint32_t reserved;
} zrt_pass_info;

int zrt_ctx_accum_begin(zrt_ctx* ctx, const zrt_camera* camera, const zrt_params* params);
int zrt_ctx_accum_pass(zrt_ctx* ctx, uint32_t n_samples, float* dev_tiles, void* hip_stream);
/* The last pass's metrics and times (waits for it). */
int zrt_ctx_accum_info(zrt_ctx* ctx, zrt_pass_info* out);

/* zrt_render in passes of pass_samples samples (rounded up to whole sample
 * chunks; 0 selects ZRT_DEFAULT_PASS_CHUNKS chunks) on one GPU
 * (params->device).  After each pass on_pass (may be NULL) receives the
 * assembled frame so far (width*height*3 f32, row 0 = bottom; it is out_rgb)
 * and the pass's info; a nonzero return stops the run.  out_rgb and stats then
 * hold the frame and the counters at info.samples_done samples per pixel: for a
 * run that was not stopped, zrt_render's. */
typedef int (*zrt_pass_fn)(void* user, const float* rgb, const zrt_pass_info* info);
/* Every pass is a launch with an end of its own, so passes cost time: the bunny
 * at 2048 x 2048, 1024 spp in passes of 1 / 2 / 4 / 8 chunks takes 81 / 34 / 15 /
 * 5.7 % longer than the single launch; no pass shorter than
 * the frame stays inside the single launch's run-to-run spread (0.2 %). */
enum { ZRT_DEFAULT_PASS_CHUNKS = 8u };
int zrt_render_progressive(const zrt_scene* scene, const zrt_camera* camera,
                           const zrt_params* params, uint32_t pass_samples,
                           zrt_pass_fn on_pass, void* user, float* out_rgb, zrt_stats* stats);

/* How zrt_ctx_accum_pass turns (params->samples_per_pixel = the cap,
 * params->sample_chunk, done, n_samples) into a launch, with no device (the
 * launch path calls the same function; it returns the refusals above). */
typedef struct zrt_pass_plan {
  uint32_t first_sample;   /* = done: the frame's sample index of the pass's sample 0 */
  uint32_t pass_samples;
  uint32_t samples_after;  /* done + n_samples */
  uint32_t chunk;          /* the sample chunk in use (sample_chunk, or 32 for 0) */
  uint32_t pass_chunks;    /* chunk sums per pixel the pass writes */
  uint32_t last_chunk;     /* samples in the last of them (< chunk: a ragged pass) */
  uint64_t partial_bytes;  /* the pass's chunk sums: this rank's tiles x 64 x pass_chunks x 16 B */
  uint64_t key_offset;     /* added to the launch's seed term: sample s of the pass draws the
                              stream of the frame's sample s + done */
} zrt_pass_plan;
int zrt_debug_pass_plan(const zrt_params* params, uint32_t done, uint32_t n_samples, zrt_pass_plan* out);

/* ---- adaptive sampling: stop refining 8x8 tiles that have converged --------- *
 * An accumulation run whose passes ("levels") cover only the tiles still active.
 *
 * Levels.  chunk is the sample chunk in use (zrt_pass_plan.chunk).  L_0 is
 * first_level rounded up to whole chunks, at least one chunk; L_k = 2 L_(k-1)
 * while that is below the cap, params->samples_per_pixel; the last level is the
 * cap itself (it may be ragged, as a run's last pass).  Level k renders samples
 * [L_(k-1), L_k) (L_(-1) = 0) of every pixel of the active tiles, as a pass does.
 * L_0 >= cap: one level, no decision, zrt_render's frame.
 *
 * Decision, after every level k >= 1 but the last, per in-frame pixel of an
 * active tile: A = the preview at L_k (the pixel's sum x 1.0f / float(L_k), as
 * every pass resolves it), H = the preview at L_(k-1); in f32, in this order,
 * nothing fused:
 *     d = (|A.r - H.r| + |A.g - H.g|) + |A.b - H.b|
 *     s = (A.r + A.g) + A.b
 *     pass = d <= tolerance * sqrtf(s)      (IEEE sqrtf; a NaN compares false)
 * With P(2n) = (P(n) + Q) / 2, Q the mean of the second half, P(2n) - P(n) =
 * (Q - P(n)) / 2 has the variance of P(2n) itself: |A - H| is a one-sample
 * estimate of the preview's standard error (the half-buffer estimate), taken
 * relative to sqrt(brightness).  A tile has converged when every in-frame pixel
 * of it passes (lanes outside the frame pass; a tile with a NaN pixel runs to
 * the cap).  A converged tile is frozen: its samples stay at L_k and its sums
 * and its pixels in dev_tiles are not touched again.  Both previews are, bit for
 * bit, full renders at L_k and L_(k-1) samples per pixel, so the decisions are a
 * function of two such frames.  The surviving tiles keep their order (the
 * scheduling probe's costliest-first order, or tile order).
 *
 * tolerance must be finite and >= 0 (ZRT_E_INVALID otherwise). */
typedef struct zrt_adaptive {
  float tolerance;
  uint32_t first_level;  /* samples per pixel of level 0 (0: one chunk) */
  uint32_t reserved[2];
} zrt_adaptive;

typedef struct zrt_level_info {
  uint32_t level_samples;       /* L_k: samples per pixel of the tiles rendered in this level */
  uint32_t tiles_rendered;      /* this rank's tiles active in the level */
  uint32_t tiles_active_after;  /* of them, still active (0 after the last level) */
  uint32_t reserved;
  uint64_t samples_rendered;    /* in-frame pixels of the rendered tiles x the level's samples */
  uint64_t changed_pixels;      /* as zrt_pass_info, over the rendered tiles */
  float    max_abs_change;
  float    render_ms;           /* probe (level 0, if scheduled) + render kernel */
  float    schedule_ms;         /* the probe + sort; 0 on every level but a scheduled run's first */
  uint32_t reserved2;
} zrt_level_info;

/* zrt_ctx_adapt_begin starts an adaptive run as zrt_ctx_accum_begin starts a
 * plain one (same validation; one run of either kind is live per context, a
 * begin of either kind restarts, a zrt_ctx_render_tiles ends it).
 *
 * zrt_ctx_adapt_level renders and resolves the next level and returns once the
 * number of surviving tiles is known: one stream wait per level, at most
 * log2(cap / L_0) + 2 levels.  out may be NULL.  dev_tiles must be the same
 * buffer for the whole run: frozen tiles keep what was last written there.
 * ZRT_E_INVALID: no live adaptive run, after the last level, or nothing active.
 * A device error is sticky as in a plain run: NaN in every tile of the rank,
 * ZRT_E_UNSUPPORTED from this and every later level.
 *
 * zrt_ctx_adapt_samples: samples per pixel of each local tile so far (per_tile:
 * cap_tiles >= zrt_ctx_tile_count entries).  zrt_ctx_stats / zrt_ctx_scanlines
 * report the run so far: samples_processed = sum over tiles of in-frame pixels x
 * samples(tile), rays_processed = samples + reflections - recursion_depth_hits
 * (counted by the kernel under ZRT_FLAG_STATS). */
int zrt_ctx_adapt_begin(zrt_ctx* ctx, const zrt_camera* camera, const zrt_params* params,
                        const zrt_adaptive* adaptive);
int zrt_ctx_adapt_level(zrt_ctx* ctx, float* dev_tiles, void* hip_stream, zrt_level_info* out);
int zrt_ctx_adapt_samples(zrt_ctx* ctx, uint32_t* per_tile, uint32_t cap_tiles);

/* zrt_render with adaptive sampling on one GPU (params->device).  After each
 * level on_level (may be NULL) receives the assembled frame so far (it is
 * out_rgb) and the level's info; a nonzero return stops the run.  out_samples
 * (may be NULL): width*height samples per pixel in the frame's layout (0 for
 * pixels outside the rendered square, x >= height). */
typedef int (*zrt_level_fn)(void* user, const float* rgb, const zrt_level_info* info);
int zrt_render_adaptive(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
                        const zrt_adaptive* adaptive, zrt_level_fn on_level, void* user, float* out_rgb,
                        uint32_t* out_samples, zrt_stats* stats);
/* zrt_render_adaptive that also returns the run's per-scanline counters, as
 * zrt_render_progress does (scanlines: params->height entries; a row's samples
 * are its tiles' own). */
int zrt_render_adaptive_progress(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
                                 const zrt_adaptive* adaptive, zrt_level_fn on_level, void* user, float* out_rgb,
                                 uint32_t* out_samples, zrt_stats* stats, zrt_scanline* scanlines);

/* The level list L_0 .. of a run with these params, with no device (the launch
 * path calls the same function; it returns the refusals above and those of
 * zrt_debug_pass_plan for the cap).  *n_levels: the number of levels; the first
 * min(cap, *n_levels) are written to levels. */
int zrt_debug_adapt_plan(const zrt_params* params, const zrt_adaptive* adaptive, uint32_t* levels,
                         uint32_t cap, uint32_t* n_levels);

/* ---- the variance plane: what a run's chunk sums say of its noise ------------ *
 * A pixel's accumulator is the sum of its chunk sums S_j (one per sample chunk,
 * added in chunk order).  The run also keeps, per pixel, in f32, nothing fused,
 * in chunk order:
 *     l_j = (S_j.r + S_j.g) + S_j.b        Q = Q + l_j * l_j        (Q = 0 at begin)
 * A ragged last chunk goes into the sums but not into Q, and a device error
 * leaves NaN in Q as in the sums.  The scatter of the l_j around their mean is an
 * unbiased estimate of the variance of the preview pixel's brightness r + g + b
 * (the s of the adaptive rule).
 *
 * zrt_ctx_accum_variance reads the live plain or adaptive run and writes one f32
 * per pixel of this rank's tiles to dev_tiles_var (a device pointer, tile-major,
 * n_tiles*64 f32: dev_tiles' layout with one channel) on hip_stream (NULL: the
 * context's own).  It waits for the run's last pass, then enqueues.  c = the
 * sample chunk in use, n = the samples in the pixel's accumulator (samples_done;
 * in an adaptive run the tile's own count, zrt_ctx_adapt_samples), k = n / c.  On
 * the host, in f32, per distinct k (per tile in an adaptive run):
 *     ik = 1.0f / float(k)        sc = 1.0f / (float(k - 1) * (float(c) * float(c)))
 * Per in-frame pixel, acc = its sums, in f32, nothing fused:
 *     M    = (acc.r + acc.g) + acc.b
 *     mean = M * ik
 *     v    = Q * ik - mean * mean ;  v = v > 0 ? v : 0      (a NaN M or Q gives NaN, not 0)
 *     var  = v * sc
 * Out-of-frame slots are 0.  Q * ik - mean * mean cancels: its relative error is
 * about k * 2^-23 * mean^2 / v, clamped at 0.
 * ZRT_E_INVALID: no live run, no pass yet, a tile with n % c != 0 (a ragged pass
 * happened) or a rendered tile with k < 2.  After a device error the plane is NaN
 * and the status is the run's sticky ZRT_E_UNSUPPORTED. */
int zrt_ctx_accum_variance(zrt_ctx* ctx, float* dev_tiles_var, void* hip_stream);

/* zrt_ctx_assemble / zrt_ctx_assemble_padded for one-channel planes: gathered
 * tile-major planes (n_tiles*64 f32 per rank; stride_tiles 0: packed rank after
 * rank, else rank r starts at tile r * stride_tiles) into the frame's layout,
 * dev_frame: width*height f32, zero outside the rendered square. */
int zrt_ctx_assemble_plane(zrt_ctx* ctx, const zrt_params* params, const float* dev_gathered,
                           uint32_t stride_tiles, float* dev_frame, void* hip_stream);

/* (c, n) -> (k, ik, sc) as zrt_ctx_accum_variance computes them, with no device
 * (the launch path calls the same function; it returns the refusals above: n == 0,
 * n % c != 0, k < 2).  Only params->sample_chunk is read beyond the validation of
 * the params; n_samples need not lie under params->samples_per_pixel. */
typedef struct zrt_variance_plan {
  uint32_t chunk;  /* c: the sample chunk in use (sample_chunk, or 32 for 0) */
  uint32_t k;      /* whole chunks in the accumulator */
  float ik;        /* 1.0f / float(k) */
  float sc;        /* 1.0f / (float(k - 1) * (float(c) * float(c))) */
} zrt_variance_plan;
int zrt_debug_variance_plan(const zrt_params* params, uint32_t n_samples, zrt_variance_plan* out);

/* ---- denoising: first-hit feature buffers and an a-trous filter ------------- *
 * A frame of few samples is noisy; an edge-avoiding a-trous wavelet filter
 * (Dammertz et al. 2010) smooths it where the surface under a pixel's
 * neighbours is the same surface.  What it knows of the surface is a feature
 * buffer: two float4 per pixel in the frame's layout (row-major, row 0 = bottom),
 *     {N.x, N.y, N.z, t}   the first hit's normal (HitRecord.normal) and t
 *     {A.r, A.g, A.b, id}  its albedo; id = the bits of uint32(prim + 1), 0: a miss
 * The filter is a pure function of (frame, features, params, zrt_denoise): the
 * features may come from anywhere.
 *
 * Definition.  All f32, nothing fused, in this order.  D = the pixels with
 * x < height and y < height (raytrace.zig:168's square); pixels outside D are
 * copied.  h = {1/16, 1/4, 3/8, 1/4, 1/16} for offsets -2 .. 2.  On the host,
 * in f32: inv_c = 1.0f / sigma_color, likewise inv_n, inv_a, inv_z.  C_0 = the
 * input.  Iteration i = 0 .. iterations - 1 has step s = 2^i and colour scale
 * kc = inv_c * float(1 << i) (sigma_color halves every iteration).  Per pixel p
 * of D: rz = 1.0f / t(p) (IEEE) if id(p) != 0, else 0; kz = inv_z * rz;
 * acc = (0, 0, 0), wsum = 0.  Then dy = -2 .. 2 (outer), dx = -2 .. 2 (inner),
 * q = p + s (dx, dy):
 *     q outside D: skip.
 *     dx = dy = 0: w = h(0) * h(0), no tests.
 *     otherwise:  (id(p) == 0) != (id(q) == 0): skip.  w = h(dx) * h(dy); for each
 *       term that is on, in the order colour, normal, albedo, depth: compute t_x,
 *       skip the tap unless t_x > 0, then w = w * t_x:
 *         t_c = 1.0f - ((|dR| + |dG|) + |dB|) * kc         d = C_i(p) - C_i(q)
 *         t_n = 1.0f - ((dNx*dNx + dNy*dNy) + dNz*dNz) * inv_n
 *         t_a = 1.0f - ((|dAr| + |dAg|) + |dAb|) * inv_a
 *         t_z = 1.0f - |t(p) - t(q)| * kz
 *       skip the tap unless w > 0.
 *     acc.c = acc.c + C_i(q).c * w per channel, then wsum = wsum + w.
 * C_(i+1)(p).c = acc.c / wsum (IEEE).  The output is C_iterations.
 * The weights are tents (1 - x, cut at 0), not exp(-x): every step is an f32
 * operation a caller can restate exactly, and the tap loop holds no
 * transcendental.  A NaN compares false: a NaN neighbour is skipped, a pixel
 * whose own colour is NaN stays NaN through the untested centre tap, so the NaN
 * frame of a device error stays recognisable. */
typedef struct zrt_denoise {
  uint32_t iterations;      /* 1..8; 0 selects ZRT_DEFAULT_DENOISE_ITERATIONS */
  float sigma_color;        /* each: finite > 0 = on, 0 = that term off (factor 1) */
  float sigma_normal;
  float sigma_albedo;
  float sigma_depth;        /* relative: a fraction of the centre pixel's depth */
  uint32_t reserved[3];
} zrt_denoise;
enum { ZRT_DEFAULT_DENOISE_ITERATIONS = 5u };

/* The default filter (host only).  The sigmas are the winner of the grid search
 * of tools/denoise_probe.py (profiles/r10/denoise/defaults.json). */
int zrt_denoise_defaults(zrt_denoise* out);

/* The feature buffer of a frame (see above) written to dev_features (a device
 * pointer, width*height*8 f32, 16-byte aligned) on hip_stream (NULL: the
 * context's own).  Asynchronous, as zrt_ctx_render_tiles; params validated the
 * same way; the whole frame whatever rank / world_size say; one ray per pixel.
 * The ray goes through the pixel centre: u = float(x) / float(width), v =
 * float(y) / float(height) - raytrace.zig:173-174's ((float)x + r - 0.5f) /
 * f_width at r = 0.5 - then Camera.getRay (camera.zig:46-51) and Ray.init.
 * The hit is rayColor's closest hit (t_min = 0.001, t_max = inf) through
 * params->traversal with the grazing-triangle guard on, as zrt_trace.  On a
 * hit: N = HitRecord.normal (the outward normal flipped against the ray), t
 * the hit's t, A the material's texture albedo at the hit's (u, v) for
 * Lambertian and metal, (1, 1, 1) for a dielectric, id = uint32(prim + 1), prim
 * the index in scene->prims.  On a miss: N = 0, t = 0, A = backgroundColor(d),
 * id = 0.  Pixels with x >= height (outside the rendered square,
 * raytrace.zig:168): all eight floats 0.  A traversal stack overflow sets the
 * context's error flag, as in a render launch (zrt_ctx_sync reports it), and
 * the buffer then holds NaN. */
int zrt_ctx_features(zrt_ctx* ctx, const zrt_camera* camera, const zrt_params* params,
                     float* dev_features, void* hip_stream);

/* Filters dev_frame into dev_out (device pointers, width*height*3 f32 each;
 * dev_out != dev_frame) guided by dev_features (width*height*8 f32, 16-byte
 * aligned) on hip_stream (NULL: the context's own).  Asynchronous; one launch
 * per iteration.  The ping-pong planes belong to the context, so one denoise
 * is in flight per context.  params gives width and height and is validated as
 * zrt_ctx_render_tiles validates it.  ZRT_E_INVALID: a negative, NaN or infinite
 * sigma, iterations > 8, height > width, dev_out == dev_frame, a null or
 * misaligned pointer. */
int zrt_ctx_denoise(zrt_ctx* ctx, const zrt_params* params, const zrt_denoise* dn,
                    const float* dev_frame, const float* dev_features,
                    float* dev_out, void* hip_stream);
/* Device time of the last zrt_ctx_denoise in ms (HIP events; waits for it). */
int zrt_ctx_denoise_ms(zrt_ctx* ctx, double* ms);

/* One-shot on one GPU (params->device): zrt_render (adaptive NULL) or
 * zrt_render_adaptive, then assemble, zrt_ctx_features and zrt_ctx_denoise on
 * the device, then the copy out.  dn NULL: zrt_denoise_defaults.  out_rgb: the
 * denoised frame; out_noisy (may be NULL): the unfiltered frame, bit for bit
 * zrt_render's / zrt_render_adaptive's; out_features (may be NULL): width*
 * height*8 f32; denoise_ms (may be NULL): the filter's device time. */
int zrt_render_denoised(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
                        const zrt_adaptive* adaptive, const zrt_denoise* dn, float* out_rgb, float* out_noisy,
                        float* out_features, zrt_stats* stats, double* denoise_ms);

/* ---- variance-guided denoising: the a-trous filter with per-pixel variance --- *
 * The filter above tells noise from an edge by one global sigma_color.  This one
 * (the spatial filter of SVGF, Schied et al. 2017) takes a per-pixel variance of
 * the brightness r + g + b - zrt_ctx_accum_variance's plane, assembled - scales
 * its colour test by the local standard deviation, and filters the variance
 * along with the colour.  With ZRT_DN_DEMODULATE it filters the frame divided by
 * the first hit's albedo, so texture detail is not treated as noise.
 *
 * Definition.  Everything of the definition above holds except what is said
 * here; all f32, nothing fused, IEEE sqrtf and `/`.  V_0 = the variance plane.
 * L(x) = (x.r + x.g) + x.b.  sigma_color is in standard deviations of L, does not
 * halve (there is no kc: the variance shrinks by itself), and 0 switches the
 * colour term off as before; on the host sc_l = sigma_color.
 *
 * Demodulation (ZRT_DN_DEMODULATE only), a_min = 2^-6, per pixel p of D with
 * id(p) != 0, A its albedo:
 *     C_0(p).c = A.c > a_min ? frame(p).c / A.c : frame(p).c          per channel
 *     am = ((A.r + A.g) + A.b) * (1.0f / 3.0f)
 *     V_0(p) = am > a_min ? V(p) / (am * am) : V(p)
 * Misses are unchanged.  After the last iteration the output's channel c is
 * multiplied by A.c under the same per-channel test and the output variance by
 * am * am under its test (a NaN albedo fails the tests: unchanged).
 *
 * Iteration i, per pixel p of D.  First the variance smoothed over 3 x 3:
 * g = 0; dy = -1 .. 1 (outer), dx = -1 .. 1 (inner), q = p + (dx, dy) (adjacent
 * pixels at every step), wt = 1/4 (dx = dy = 0), 1/8 (dx = 0 or dy = 0), else 1/16:
 *     g = g + (q in D ? V_i(q) : V_i(p)) * wt
 * Then, with the colour term on, kl = 1.0f / (sigma_color * sqrtf(g) + 0x1p-20f).
 * vacc = 0 beside acc and wsum.  The taps are the definition's, with
 *     t_c = 1.0f - |L(C_i(p)) - L(C_i(q))| * kl
 * and a tap that survives with weight w also adds vacc = vacc + V_i(q) * (w * w)
 * after wsum = wsum + w; the centre tap adds V_i(p) * (w0 * w0), w0 = h(0) * h(0).
 *     C_(i+1)(p).c = acc.c / wsum        V_(i+1)(p) = vacc / (wsum * wsum)
 * The outputs are C_iterations and V_iterations (the variance left in the
 * filtered frame, under the assumption of independent pixels); pixels outside D
 * are copied in both.
 *
 * NaN.  A NaN variance at p or beside it makes g and kl NaN, so every tested tap
 * of p fails and p keeps its own colour through the untested centre tap; a NaN
 * variance reached by a surviving tap makes V_(i+1)(p) NaN, and p's taps fail
 * from the next iteration on.  Colours never become NaN through the variance:
 * the NaN-frame behaviour of the filter above carries over.  (With the colour
 * term off the variance guides nothing and is only filtered.) */
enum { ZRT_DN_DEMODULATE = 1u };

/* The default guided filter and flags (host only): the winner of the search of
 * tools/denoise_guided_probe.py (profiles/r11/guided/defaults.json). */
int zrt_denoise_guided_defaults(zrt_denoise* out, uint32_t* flags);

/* zrt_ctx_denoise with the definition above.  dev_variance: width*height f32 in
 * the frame's layout; dev_out_variance (may be NULL): the same, written with
 * V_iterations.  ZRT_E_INVALID: what zrt_ctx_denoise refuses, a null dev_variance,
 * dev_out_variance == dev_variance, an unknown flag.  zrt_ctx_denoise_ms reports
 * the last filter of either kind. */
int zrt_ctx_denoise_guided(zrt_ctx* ctx, const zrt_params* params, const zrt_denoise* dn, uint32_t flags,
                           const float* dev_frame, const float* dev_features, const float* dev_variance,
                           float* dev_out, float* dev_out_variance, void* hip_stream);

/* zrt_render_denoised with the guided filter.  The noisy frame is rendered as an
 * accumulation run of one pass (adaptive NULL) or as the adaptive run, so
 * out_noisy stays bit for bit zrt_render's / zrt_render_adaptive's; then
 * zrt_ctx_accum_variance, both assembles, zrt_ctx_features and
 * zrt_ctx_denoise_guided.  dn NULL: zrt_denoise_guided_defaults' filter (flags
 * are the caller's either way).  out_variance (may be NULL): width*height f32,
 * the noisy frame's variance plane.  ZRT_E_INVALID before any device work when
 * samples_per_pixel is not a multiple of the sample chunk or holds fewer than two
 * chunks: choose a smaller params->sample_chunk. */
int zrt_render_denoised_guided(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
                               const zrt_adaptive* adaptive, const zrt_denoise* dn, uint32_t flags, float* out_rgb,
                               float* out_noisy, float* out_features, float* out_variance, zrt_stats* stats,
                               double* denoise_ms);

/* ---- temporal accumulation: the last frame reprojected under a moving camera --- *
 * The filters above treat a frame as the only frame there is.  This step (the
 * temporal half of SVGF, Schied et al. 2017) finds, for every pixel, where its
 * first-hit surface point was in the previous frame of the same scene, decides
 * from the feature buffers whether that history shows the same surface, and blends
 * the history into the frame.  The variance plane is propagated through the blend
 * exactly, so zrt_ctx_denoise_guided's colour test tightens by itself on the
 * accumulated frame.  A context keeps the state: the previous camera, and per
 * pixel of D the previous features, a history {r, g, b, V} and a history length.
 *
 * The reprojection plan (host, f32, nothing fused).  o, llc, H, W = the previous
 * camera's origin, lower_left_corner, horizontal, vertical; b = llc - o;
 *     cross(a, c) = (a.y*c.z - a.z*c.y, a.z*c.x - a.x*c.z, a.x*c.y - a.y*c.x)
 *     dot(a, c)   = (a.x*c.x + a.y*c.y) + a.z*c.z
 *     rn = cross(W, H)    ru = cross(b, W)    rv = cross(H, b)    s = dot(b, rn)
 * Camera.init's vectors give s > 0 (H x W points backwards, W x H forwards); s < 0 - a
 * left-handed camera - negates rn, ru and rv.  s == 0 or NaN: valid = 0, and a temporal
 * call with such a plan has no history.
 * A point P = o + l (b + u H + v W) has d = P - o with dot(d, rn) = l |s|,
 * dot(d, ru) = l u |s|, dot(d, rv) = l v |s|: it lies in front of the previous
 * camera iff den = dot(d, rn) > 0, at the pixel coordinates
 *     fx = (dot(d, ru) / den) * float(width)    fy = (dot(d, rv) / den) * float(height)
 * (pixel centres are the integers: zrt_ctx_features shoots pixel x at u = float(x) /
 * float(width)). */
typedef struct zrt_reproject_plan {
  zrt_vec3 origin;  /* o */
  zrt_vec3 rn, ru, rv;
  float s;          /* dot(b, rn) before the sign rule */
  uint32_t valid;
} zrt_reproject_plan;
/* Only params->width / height are read beyond the validation of the params (they
 * scale fx / fy in the kernel; the plan's vectors do not depend on them). */
int zrt_debug_reproject_plan(const zrt_camera* prev, const zrt_params* params, zrt_reproject_plan* out);

/* Definition.  All f32, nothing fused, IEEE `/` and sqrtf, in this order.  D, the
 * feature buffer, a_min = 2^-6 and the demodulation rule are the guided filter's.
 * n_D = height.  On the host inv_n = 1.0f / sigma_normal, inv_z = 1.0f / sigma_depth
 * for the terms that are on.  Pixels outside D are copied (colour and variance),
 * their length is 0 and they are never a tap.  Per pixel p = (x, y) of D:
 *  1. c = frame(p), v = variance(p).  With ZRT_TA_DEMODULATE and id(p) != 0:
 *     c.c = A.c > a_min ? c.c / A.c : c.c per channel, am = ((A.r + A.g) + A.b) *
 *     (1.0f / 3.0f), v = am > a_min ? v / (am * am) : v.  The history then holds
 *     demodulated values.
 *  2. No history - out = c, outv = v, n = 1 - when the context holds no state (the
 *     first call, after zrt_ctx_temporal_reset, after a change of width, height or
 *     ZRT_TA_DEMODULATE, a previous camera whose plan has valid = 0) or id(p) == 0:
 *     the background is a function of the direction and carries no noise.
 *  3. Where the point was.  The camera equal to the previous one byte for byte
 *     (decided on the host): fx = float(x), fy = float(y), te = t(p).  Otherwise the
 *     pixel-centre ray as zrt_ctx_features builds it: u = float(x) / float(width),
 *     v = float(y) / float(height), e = ((llc + H * u) + W * v) - o per component
 *     (camera.zig:46-51), dir = e / sqrtf((e.x*e.x + e.y*e.y) + e.z*e.z) (Ray.init);
 *     P = o + dir * t(p) per component (ray.zig:14-16); d = P - o_prev; den, fx, fy
 *     as above; te = sqrtf(dot(d, d)); and there is no history unless den > 0,
 *     fx > -1.0f, fx < float(n_D), fy > -1.0f, fy < float(n_D) (a NaN fails).
 *  4. x0f = floorf(fx), a = fx - x0f, likewise y0f, bb; kz = inv_z * (1.0f / te).
 *     nmin = 2^32 - 1.  Four taps (i, j) = (0,0), (1,0), (0,1), (1,1) at q = (x0 + i,
 *     y0 + j) with w = (i ? a : 1.0f - a) * (j ? bb : 1.0f - bb).  A tap is skipped
 *     unless q is in D, w > 0, len(q) != 0, id_prev(q) != 0, with the normal term
 *     on 1.0f - ((dNx*dNx + dNy*dNy) + dNz*dNz) * inv_n > 0 for dN = N(p) - N_prev(q),
 *     with the depth term on 1.0f - |te - t_prev(q)| * kz > 0, and no lane of the
 *     history {r, g, b, V} at q is NaN.  A surviving tap adds acc.c = acc.c +
 *     Hc(q).c * w, vacc = vacc + Hv(q) * w, wsum = wsum + w, nmin = min(nmin, len(q)).
 *     Surface ids are not compared: adjacent triangles of one mesh differ in id.
 *  5. No tap survived: as in 2.  Else h.c = acc.c / wsum, hv = vacc / wsum,
 *     n = min(nmin + 1, max_history), r = 1.0f / float(n), al = r > alpha_min ? r :
 *     alpha_min, om = 1.0f - al, out.c = h.c * om + c.c * al,
 *     outv = hv * (om * om) + v * (al * al).
 *  6. The history at p becomes {out, outv}, len(p) = n, and the previous features
 *     at p the features at p.  The outputs are out - with ZRT_TA_DEMODULATE and
 *     id(p) != 0 channel c times A.c where A.c > a_min - outv (times am * am where
 *     am > a_min) and n.
 * The variance line of step 5 assumes the history and the frame are independent:
 * change params->seed from frame to frame.  The bilinear weights interpolate the
 * history's variance as a value; they do not claim its taps are independent.
 * NaN: a NaN pixel of the frame gives a NaN output and a NaN history entry, which
 * the next frame skips as a tap - the NaN frame of a device error stays
 * recognisable and does not outlive one frame. */
typedef struct zrt_temporal {
  float alpha_min;       /* in [0, 1]: the least weight of the new frame in the blend */
  uint32_t max_history;  /* 1 .. 65535; 0 selects ZRT_DEFAULT_TEMPORAL_HISTORY */
  float sigma_normal;    /* each: finite > 0 = on, 0 = that test off */
  float sigma_depth;     /* relative: a fraction of the reprojected distance te */
  uint32_t flags;        /* ZRT_TA_* */
  uint32_t reserved[3];
} zrt_temporal;
enum { ZRT_TA_DEMODULATE = 1u };
enum { ZRT_DEFAULT_TEMPORAL_HISTORY = 32u };

/* The default temporal step (host only): the winner of the grid search of
 * tools/temporal_probe.py (profiles/r12/temporal/defaults.json). */
int zrt_temporal_defaults(zrt_temporal* out);

/* One frame of the definition above on hip_stream (NULL: the context's own).
 * Asynchronous, one launch; the state belongs to the context, so the calls of a
 * sequence go to one stream (or to streams the caller orders).  camera and params:
 * what dev_features was made with.  dev_frame, dev_out: width*height*3 f32;
 * dev_features: width*height*8 f32, 16-byte aligned; dev_variance: width*height f32;
 * dev_out_variance (may be NULL): the same; dev_out_len (may be NULL): width*height
 * uint32.  The state is allocated on first use and again when width or height
 * change.  ZRT_E_INVALID: what zrt_ctx_denoise_guided refuses of its pointers and
 * params, alpha_min outside [0, 1] or NaN, a negative, NaN or infinite sigma,
 * max_history > 65535, an unknown flag, dev_out == dev_frame. */
int zrt_ctx_temporal(zrt_ctx* ctx, const zrt_camera* camera, const zrt_params* params, const zrt_temporal* tp,
                     const float* dev_frame, const float* dev_features, const float* dev_variance,
                     float* dev_out, float* dev_out_variance, uint32_t* dev_out_len, void* hip_stream);
/* Drops the history: the next zrt_ctx_temporal is a first call. */
int zrt_ctx_temporal_reset(zrt_ctx* ctx);
/* Device time of the last zrt_ctx_temporal in ms (HIP events; waits for it). */
int zrt_ctx_temporal_ms(zrt_ctx* ctx, double* ms);

/* A sequence of n_frames frames of one scene on one GPU (params->device), cameras[k]
 * the camera of frame k.  Frame k: an accumulation run of one pass with seed
 * params->seed + k, zrt_ctx_accum_variance, both assembles, zrt_ctx_features,
 * zrt_ctx_temporal (tp NULL: zrt_temporal_defaults), then zrt_ctx_denoise_guided
 * on its colour and variance (dn NULL: the guided defaults' filter; dn_flags are
 * the caller's either way).  on_frame (may be NULL) receives each filtered frame
 * (width*height*3 f32; it is out_rgb) and its index; a nonzero return stops the
 * sequence.  out_rgb: the last filtered frame; stats (may be NULL): the last
 * frame's.  ZRT_E_INVALID before any device work: zrt_render_denoised_guided's
 * refusal of a ragged or single-chunk samples_per_pixel, n_frames == 0, and what
 * zrt_ctx_temporal refuses of tp. */
typedef int (*zrt_frame_fn)(void* user, const float* rgb, uint32_t frame);
int zrt_render_temporal(const zrt_scene* scene, const zrt_camera* cameras, uint32_t n_frames,
                        const zrt_params* params, const zrt_temporal* tp, const zrt_denoise* dn, uint32_t dn_flags,
                        zrt_frame_fn on_frame, void* user, float* out_rgb, zrt_stats* stats);

/* ---- ray queries: closest hit and any hit on a resident context -------------- *
 * zrt_trace builds the BVH, uploads and tears down for every batch.  These calls
 * ask the scene a zrt_ctx already holds: device pointers, a stream (NULL: the
 * context's own), asynchronous as zrt_ctx_features.  params supplies traversal,
 * device and bounded_volume_hierarchy, which must fit the context (ZRT_E_INVALID
 * otherwise); every traversal and the surface list (no BVH) are served.  Rays are
 * n x {origin xyz, direction xyz}; Ray.init normalises the direction
 * (ray.zig:11-13).  n == 0: ZRT_OK, nothing is enqueued.  A null or misaligned
 * (4-byte) pointer: ZRT_E_INVALID.  A query has deep stack rows, an error flag and a
 * completion of its own, so it disturbs neither a render or accumulation run nor a
 * feature launch on the same context; one query is in flight per context.  A
 * traversal stack overflow is reported by zrt_ctx_sync, or by the next call that
 * looks at the context's launches, as ZRT_E_UNSUPPORTED (once); the outputs of
 * that launch are overwritten: t = NaN, prim = -1, every occlusion byte = 0xFF.
 *
 * "Occluded" is what the reference's own code returns: the top-level surface loop
 * of rayColor (raytrace.zig:71-81) started with t_min = 0.001 and t_max = the
 * caller's value instead of +inf, as closest_hit != null.  Over the list: some
 * primitive's hit(ray, 0.001, t_max) is non-null; the bounds are strict (t < t_max,
 * sphere.zig:43/57, triangle.zig:62).  Under the BVH it is BVHNode.hit(ray, 0.001,
 * t_max) (bvh.zig:187-205): until the first hit t_max never shrinks and after it
 * the answer is "yes", so it equals: some leaf whose box, and all of whose
 * ancestors' boxes, pass hitAabb(ray, 0.001, t_max) (aabb.zig:109-127, each axis on
 * its own) holds a primitive that hits in (0.001, t_max).  That is neither "some
 * primitive is hit below t_max" nor "the closest hit lies below t_max": a rounded
 * hit can lie outside its own leaf's box, and a finite t_max clips slabs the
 * infinite one lets through (DESIGN.md section 5 "Ray queries").  Every traversal
 * returns this answer; FAST walks the full 128-B wide nodes (any-hit has no flavour
 * over the compressed ones) with the grazing-triangle guard on, as zrt_trace.  A
 * t_max that is NaN or <= 0.001 gives 0. */

/* Closest hit of n rays on a resident context: zrt_trace's query, with device pointers,
 * on a stream, asynchronous.  dev_rays: n x {origin xyz, direction xyz}; dev_t: n f32
 * (+inf on a miss); dev_prim: n i32, index into scene->prims (-1 on a miss), mapped on the device. */
int zrt_ctx_trace(zrt_ctx* ctx, const zrt_params* params, const float* dev_rays, uint32_t n,
                  float* dev_t, int32_t* dev_prim, void* hip_stream);

/* Any hit in (0.001, t_max): what rayColor's surface loop (raytrace.zig:71-81) returns when started
 * with t_max instead of +inf, as != null.  dev_t_max: n f32, or NULL = +inf for every ray.
 * dev_out: n bytes, 1 occluded / 0 not. */
int zrt_ctx_occluded(zrt_ctx* ctx, const zrt_params* params, const float* dev_rays, const float* dev_t_max,
                     uint32_t n, uint8_t* dev_out, void* hip_stream);

/* One-shot, host pointers, like zrt_trace. */
int zrt_occluded(const zrt_scene* scene, const zrt_params* params, const float* rays, const float* t_max,
                 uint32_t n, uint8_t* out);

/* ms between the events around the last query launch of the context (as zrt_ctx_denoise_ms). */
int zrt_ctx_query_ms(zrt_ctx* ctx, double* ms);

/* ---- ambient occlusion: cosine rays from the first hits, exact any-hit ---------- *
 * The reference has no lights, so ambient occlusion is the one visibility plane that
 * is defined in its own terms: an AO ray is exactly the ray Lambertian.scatter shoots
 * (material.zig:71-75) - origin HitRecord.location, direction normal +
 * randomUnitVector, cosine-distributed by construction.  One fused kernel turns a
 * feature buffer (zrt_ctx_features) into per-pixel counts of rays that got away; no ray
 * is ever stored.  AO is a pure function of (features, camera, params, zrt_ao).
 *
 * All f32, nothing fused, IEEE `/`.  D is the set of pixels with x < height.  Per
 * pixel p = (x, y), with N(p), t(p), id(p) from dev_features:
 *   p outside D      clear = 0, ao = 0, on every call, with or without ZRT_AO_ACCUMULATE.
 *   id(p) == 0       (a miss) no ray is shot, c = n_samples.
 *   a lane of N(p) or t(p) is NaN   (the NaN buffer of a device error) clear =
 *                    0xFFFFFFFF, ao = NaN; under ZRT_AO_ACCUMULATE a plane value of
 *                    0xFFFFFFFF stays 0xFFFFFFFF (and ao NaN), on any pixel.
 *   otherwise        the pixel-centre ray as zrt_ctx_features builds it: u = float(x) /
 *                    float(width), v = float(y) / float(height), e = ((llc + H u) + W v)
 *                    - o, dir = e / sqrtf((e.x e.x + e.y e.y) + e.z e.z); P = o + dir
 *                    t(p) per component (ray.zig:14-16).  For s = first_sample ..
 *                    first_sample + n_samples - 1: key = ((uint64(y) width + x) << 16 |
 *                    s) + seed 0x9E3779B97F4A7C15 (the counter mode's key), rng =
 *                    DefaultPrng.init(key) of params->prng, r = randomUnitVector(rng)
 *                    (sample.zig:47-61, the first draws of the stream), d = N(p) + r
 *                    (material.zig:73), the ray Ray.init(P, d), which normalises;
 *                    "occluded" is zrt_ctx_occluded's definition for that ray at t_max
 *                    = radius through params->traversal.  A d that normalises to NaN is
 *                    not occluded.  c = the samples that are not occluded.
 * Without ZRT_AO_ACCUMULATE clear(p) = c and ao(p) = float(c) / float(n_samples); with
 * it clear(p) = clear(p) + c and ao(p) = float(clear(p)) / float(first_sample +
 * n_samples): the caller's plane holds the counts of samples [0, first_sample).  Counts
 * are integers, so calls over [0, 8) and [8, 16) equal one call over [0, 16).
 *
 * dev_features: width * height * 8 f32, 16-byte aligned; dev_clear: width * height u32
 * in the frame's layout; dev_ao: width * height f32, or NULL.  Asynchronous on
 * hip_stream (NULL: the context's own).  params is validated as zrt_ctx_features
 * validates it; traversal, prng, seed, width, height, device and
 * bounded_volume_hierarchy are read.  ZRT_E_INVALID before any device work: n_samples
 * == 0 or > 1024, first_sample + n_samples > 65536 (the key's sample field), a radius
 * that is NaN or <= 0.001, an unknown flag, a null dev_features / dev_clear, a
 * misaligned pointer, height > width, params that do not fit the context.
 *
 * AO is a query (see "ray queries"): its rows, error flag, completion and events are
 * the query's, zrt_ctx_query_ms times its kernel.  After a traversal stack overflow
 * every count of D holds 0xFFFFFFFF and every ao of D NaN, and zrt_ctx_sync reports
 * ZRT_E_UNSUPPORTED once. */
typedef struct zrt_ao {
  uint32_t n_samples;     /* AO rays per pixel in this call, 1 .. 1024 */
  uint32_t first_sample;  /* index of this call's sample 0 in the pixel's AO stream */
  float    radius;        /* t_max of every AO ray: > 0.001, +inf allowed */
  uint32_t flags;         /* ZRT_AO_* */
  uint32_t reserved[4];
} zrt_ao;
enum { ZRT_AO_ACCUMULATE = 1u };

int zrt_ctx_ao(zrt_ctx* ctx, const zrt_camera* camera, const zrt_params* params, const zrt_ao* ao,
               const float* dev_features, uint32_t* dev_clear, float* dev_ao, void* hip_stream);

/* ms between the events around the last AO kernel of the context: zrt_ctx_query_ms. */
int zrt_ctx_ao_ms(zrt_ctx* ctx, double* ms);

/* One-shot, host pointers: a context, the features, the AO call, the copies out.  out_ao:
 * width * height f32; out_clear (width * height u32) and out_features (width * height * 8
 * f32) may be NULL.  Under ZRT_AO_ACCUMULATE out_clear is read first: its contents are the
 * counts of samples [0, first_sample) the call adds onto (NULL: zeros). */
int zrt_render_ao(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params, const zrt_ao* ao,
                  float* out_ao, uint32_t* out_clear, float* out_features);

/* How zrt_ctx_ao launches (no device; the launch path calls the same function): a lane
 * is one (pixel, sample), pixels in 8x8 tile order over the whole width, a pixel's
 * samples on adjacent lanes.  The grid is bounded by the CU count and each block loops
 * over its groups of 256 rays, so the stack's overflow rows are sized by the resident
 * lanes, never by the rays.  Refuses what zrt_ctx_ao refuses of params and ao. */
enum { ZRT_AO_REDUCE_WAVE = 0, ZRT_AO_REDUCE_ATOMIC = 1 };
typedef struct zrt_ao_plan {
  uint64_t rays;            /* pixel slots (tiles x 64) x n_samples */
  uint64_t groups;          /* groups of 256 rays */
  uint64_t pixel_slots;     /* tiles over the whole width x 64 */
  uint64_t resident_lanes;  /* grid x 256: the stride and the count of the overflow rows' lanes */
  uint64_t ovf_row_bytes;   /* one overflow row of 32-bit entries: resident_lanes x 4 */
  uint64_t plane_bytes;     /* the count plane of ZRT_AO_REDUCE_ATOMIC (width x height u32), else 0 */
  uint32_t grid;            /* blocks launched: min(groups, blocks_per_cu x cu_count) */
  uint32_t blocks_per_cu;
  uint32_t reduction;       /* ZRT_AO_REDUCE_WAVE: n_samples divides 64, a pixel's samples lie in one wave (one
                               ballot + popcount, the segment's first lane writes); else ZRT_AO_REDUCE_ATOMIC:
                               vector atomic adds on a zeroed count plane, folded in by the finishing kernel */
  uint32_t reserved;
} zrt_ao_plan;
int zrt_debug_ao_plan(const zrt_params* params, const zrt_ao* ao, uint32_t cu_count, zrt_ao_plan* out);

/* ---- radiance queries: rayColor along caller-supplied rays -------------------- *
 * The last member of the query family: what colour rayColor returns along a ray, so a
 * caller can bring any camera (orthographic, fisheye, thin lens, a panorama, light
 * probes, irradiance at surface points) as a buffer of rays.  Inputs are n rays {origin
 * xyz, direction xyz} as zrt_ctx_trace takes them; Ray.init normalises the direction
 * (ray.zig:11-13).  Ray i of a call has index R = first_ray + i, a 64-bit value with
 * first_ray + n <= 2^48.  For sample s = first_sample .. first_sample + n_samples - 1 of
 * ray R:
 *   key = ((R << 16) | s) + seed * 0x9E3779B97F4A7C15   (the counter mode's key, R in the
 *                                                        pixel's place)
 *   rng = DefaultPrng.init(key) of params->prng
 *   two floats are drawn and dropped                     (the pixel jitter of raytrace.zig:173-174)
 *   col = rayColor(Ray.init(origin, direction), max_depth) on that stream (raytrace.zig:62-100)
 * Dropping the two floats makes ray R the pixel with offset R of a frame whose camera
 * maps every pixel onto that ray (horizontal = vertical = 0, origin = o,
 * lower_left_corner = o + d): the oracle's own pixel, chunking and counters included.
 *
 * Traversal: params->traversal selects it; the surface list is used without a BVH; FAST
 * walks the full 128-B nodes with the grazing-triangle guard on, as the other queries.
 * Chunks: c is the sample chunk in use (sample_chunk, or 32 for 0).  Chunk j of the call
 * holds samples first_sample + j c ..; its sum S_j is taken sequentially from 0 in sample
 * order; the last chunk may be ragged.  sum = ((sum0 + S_0) + S_1) + ... per channel, in
 * f32 with nothing fused.  Without ZRT_RQ_ACCUMULATE sum0 = 0; with it sum0 is the
 * caller's dev_sum and first_sample % c == 0 is required, so calls over [0, 8) and
 * [8, 16) at c = 4 or 8 equal one call over [0, 16) bit for bit.  rgb = sum * (1.0f /
 * float(N)) per channel (raytrace.zig:157, 182), N = n_samples, or first_sample +
 * n_samples under the flag.
 *
 * dev_rays: n * 6 f32; dev_sum: n float4 {r, g, b, 0}, 16-byte aligned; dev_rgb: n * 3
 * f32, or NULL.  Asynchronous on hip_stream (NULL: the context's own).  n == 0: ZRT_OK,
 * nothing is enqueued.  params is validated as the queries validate it; traversal, prng,
 * seed, max_depth, sample_chunk, device and bounded_volume_hierarchy are read; width,
 * height, samples_per_pixel and flags are not.  ZRT_E_INVALID before any device work:
 * n_samples == 0, first_sample + n_samples > 65536 (the key's sample field), first_ray +
 * n > 2^48, an unknown flag, ZRT_RQ_ACCUMULATE with first_sample % c != 0, a null or
 * misaligned pointer (dev_rays, dev_rgb: 4 bytes), params that do not fit the context.
 *
 * It is a query (see "ray queries"): its stack and attenuation rows, counters, error
 * flag, completion and events are the query's; it disturbs no render, run, feature
 * launch or zrt_ctx_stats; one query is in flight per context.  After a traversal stack
 * overflow every sum.rgb and rgb of the call is NaN, zrt_ctx_sync reports
 * ZRT_E_UNSUPPORTED once, and the context stays usable. */
enum { ZRT_RQ_ACCUMULATE = 1u };
/* (A struct tag only, no typedef: the one-shot entry point below bears the same name, and a
 * tag and a function share it in C and in C++; write `struct zrt_radiance`.) */
struct zrt_radiance {
  uint32_t n_samples;     /* samples per ray in this call, >= 1 */
  uint32_t first_sample;  /* index of this call's sample 0 in the ray's stream */
  uint64_t first_ray;     /* R of the call's ray 0 */
  uint32_t flags;         /* ZRT_RQ_* */
  uint32_t reserved[3];
};
/* The last radiance call of the context (waits for it).  rays = samples + reflections -
 * recursion_depth_hits: every sample traces a ray unless max_depth is 0, and every
 * scatter one more unless the depth has run out.  kernel_ms: between the events around
 * the call's kernels (zrt_ctx_query_ms). */
typedef struct zrt_radiance_info {
  uint64_t samples, rays, reflections, background_hits, recursion_depth_hits;
  double kernel_ms;
} zrt_radiance_info;
int zrt_ctx_radiance(zrt_ctx* ctx, const zrt_params* params, const struct zrt_radiance* rq, const float* dev_rays,
                     uint32_t n, float* dev_sum, float* dev_rgb, void* hip_stream);
int zrt_ctx_radiance_info(zrt_ctx* ctx, zrt_radiance_info* out);
/* Tests: of the last radiance call of the context (waits for it) - out[0] the attenuation
 * rows its plan kept in LDS, out[1] the most rows any of its paths pushed (more than
 * out[0]: rows in global memory were used), out[2] the stack rows in LDS, out[3] its grid. */
int zrt_ctx_debug_radiance(zrt_ctx* ctx, uint32_t out[4]);

/* One-shot, host pointers: a context, the call, the copies out.  sum (n float4) is read
 * first under ZRT_RQ_ACCUMULATE (NULL: zeros) and written back; it, out_rgb (n * 3 f32)
 * and info may be NULL. */
int zrt_radiance(const zrt_scene* scene, const zrt_params* params, const struct zrt_radiance* rq, const float* rays,
                 uint32_t n, float* sum, float* out_rgb, zrt_radiance_info* info);

/* How zrt_ctx_radiance launches (no device; the launch path calls the same function).  A
 * work item is one (ray, chunk).  The call's chunks are served in rounds; within a round
 * item k is ray k % n of the round's chunk k / n, so a wave holds 64 consecutive items,
 * rays of one chunk wherever n is a multiple of 64.  The grid is bounded by the CU count
 * and each block loops over its items with 64-bit indices, so the stack's and the
 * attenuation's overflow rows are sized by the resident lanes, never by the rays.  The
 * chunk sums of a round are parked in [chunk][ray]; a finishing kernel folds them into
 * dev_sum in chunk order.  Rounds keep the parked sums under partial_cap_bytes (0: the
 * default, 256 MiB; one chunk of every ray is parked whatever the cap).  Refuses what
 * zrt_ctx_radiance refuses of params, rq and n.  The launch reads ZRT_RADIANCE_PARTIAL_CAP
 * (bytes) and ZRT_RADIANCE_GRID (blocks) from the environment: test knobs, like
 * ZRT_DEBUG_STACK_CAP. */
typedef struct zrt_radiance_plan {
  uint64_t items;           /* n x call_chunks */
  uint64_t partial_bytes;   /* the parked sums of one round: n x chunks_per_round x 16 */
  uint64_t resident_lanes;  /* grid x 256: the stride and the count of the overflow rows' lanes */
  uint64_t key_offset;      /* (first_ray << 16) + seed * 0x9E3779B97F4A7C15: key = ((i << 16) | s) + key_offset */
  uint32_t chunk;           /* c */
  uint32_t call_chunks;     /* ceil(n_samples / c) */
  uint32_t last_chunk;      /* samples of the call's last chunk, 1 .. c */
  uint32_t chunks_per_round, rounds;
  uint32_t grid;            /* blocks launched for a full round: min(ceil(n x chunks_per_round / 256), blocks_per_cu x cu_count) */
  uint32_t blocks_per_cu;
  uint32_t reserved;
} zrt_radiance_plan;
int zrt_debug_radiance_plan(const zrt_params* params, const struct zrt_radiance* rq, uint32_t n, uint32_t cu_count,
                            uint64_t partial_cap_bytes, zrt_radiance_plan* out);

/* Rays of an equirectangular panorama from a point (host only): width * height * 6 f32,
 * pixel (x, y) at index y * width + x, row 0 the bottom.  phi = 2 pi (x + 0.5) / width,
 * theta = pi (y + 0.5) / height measured from -y; d = (sin(theta) cos(phi), -cos(theta),
 * sin(theta) sin(phi)), computed in double and rounded to f32; the origin is copied
 * unchanged. */
int zrt_rays_equirect(const float origin[3], uint32_t width, uint32_t height, float* out_rays);

/* ---- camera queries: frames through device-generated lens rays ------------------ *
 * A radiance query shoots the same ray for every sample of ray R.  A camera query
 * generates the primary ray of every sample on the device, from a lens model, and uses
 * the two jitter floats: antialiased frames of any of the models below, depth of field,
 * and any window of a frame, with the radiance query's chunked sums, accumulation and
 * counters.
 *
 * A call renders the pixel rectangle {x0, y0, w, h} of a width x height frame (width and
 * height from params, each 1 .. 65535; the whole width is addressable: raytrace.zig:168's
 * square is not applied).  Pixel (x, y) has index R = y * width + x.  Sample s = first_sample
 * .. first_sample + n_samples - 1 of it draws
 *   key  = ((R << 16) | s) + seed * 0x9E3779B97F4A7C15    (the counter mode's key of that
 *                                                          pixel: the render's own)
 *   rng  = DefaultPrng.init(key) of params->prng
 *   r1, r2 = two floats from rng                           (used, not dropped)
 *   u = ((float(x) + r1) - 0.5f) / float(width)            (IEEE /, raytrace.zig:173-174)
 *   v = ((float(y) + r2) - 0.5f) / float(height)
 *   (o, tgt) = model(u, v);  dir = tgt - o per component
 *   col = rayColor(Ray.init(o, dir), max_depth), continuing on rng
 * A model that needs lens samples draws them from a second stream,
 * DefaultPrng.init(key ^ 0xD1B54A32D192ED03), before rng is initialised.
 * All model arithmetic is f32, nothing fused, in the order written;
 * P(u, v) = (lower_left_corner + horizontal * u) + vertical * v (Camera.getRay,
 * camera.zig:47-49).
 *   ZRT_LENS_PINHOLE   o = origin, tgt = P(u, v): raytrace.zig:173-175, so on the square the
 *                      render covers the frame is oracle_render's bit for bit.
 *   ZRT_LENS_THIN      pairs a = 2 f - 1, b = 2 f' - 1 from the lens stream until
 *                      a a + b b < 1; o = (origin + axis_u * a) + axis_v * b (the lens axes
 *                      scaled by the lens radius); tgt = P(u, v): the plane is the focal plane.
 *   ZRT_LENS_ORTHO     o = P(u, v), tgt = o + axis_w.
 *   ZRT_LENS_EQUIRECT  phi = 6.2831855f * u, theta = 3.1415927f * v; sin and cos as the
 *                      reference's std.math.sin / cos; d = (sin(theta) cos(phi), -cos(theta),
 *                      sin(theta) sin(phi)) (zrt_rays_equirect's axes); o = origin, tgt = o + d.
 *   ZRT_LENS_FISHEYE   equidistant, no masking outside the image circle: px = 2 u - 1,
 *                      py = 2 v - 1, r = sqrtf(px px + py py), th = r * half_fov; r == 0:
 *                      d = axis_w, else k = sin(th) / r, d = ((axis_u * (px * k)) + axis_v *
 *                      (py * k)) + axis_w * cos(th); o = origin, tgt = o + d.
 *
 * Traversal, chunks, sums, means, ZRT_CQ_ACCUMULATE and the counters are zrt_ctx_radiance's
 * word for word, with the pixel in the ray's place: rgb = sum * (1.0f / float(N)).
 * dev_sum (width * height float4, 16-byte aligned) and dev_rgb (width * height * 3 f32, or
 * NULL) are whole-frame buffers indexed by R, row 0 at the bottom: dev_rgb is a frame as
 * zrt_image_write_png and zrt_ctx_denoise take it.  Pixels outside the rectangle are not
 * touched.  Asynchronous on hip_stream (NULL: the context's own); it is a query: one is in
 * flight per context, and after a traversal stack overflow the rectangle's pixels are NaN,
 * zrt_ctx_sync reports ZRT_E_UNSUPPORTED once, and the context stays usable.
 * params: width, height, traversal, prng, seed, max_depth, sample_chunk, device and
 * bounded_volume_hierarchy are read.  ZRT_E_INVALID before any device work: an empty
 * rectangle or one that leaves the frame, an unknown kind or flag, a non-finite descriptor
 * float, half_fov <= 0 (read by the fisheye alone, checked for every kind), n_samples == 0,
 * first_sample + n_samples > 65536, ZRT_CQ_ACCUMULATE with first_sample % c != 0, a null or
 * misaligned pointer, a slot count (8 x 8 tiles over the rectangle x 64) of 2^32 or more,
 * params that do not fit the context. */
enum { ZRT_LENS_PINHOLE = 0, ZRT_LENS_THIN = 1, ZRT_LENS_ORTHO = 2, ZRT_LENS_EQUIRECT = 3, ZRT_LENS_FISHEYE = 4 };
enum { ZRT_CQ_ACCUMULATE = 1u };
typedef struct zrt_lens {
  uint32_t kind;                                            /* ZRT_LENS_* */
  zrt_vec3 origin, lower_left_corner, horizontal, vertical; /* the view (or focal) plane, as zrt_camera */
  zrt_vec3 axis_u, axis_v, axis_w;                          /* thin: lens axes x radius; ortho, fisheye: the frame */
  float half_fov;                                           /* fisheye: radians from the axis at |p| = 1; > 0 */
  uint32_t reserved[2];
} zrt_lens;
typedef struct zrt_camera_query {
  uint32_t x0, y0, w, h;   /* the rectangle, inside the frame, not empty */
  uint32_t n_samples;      /* samples per pixel in this call, >= 1 */
  uint32_t first_sample;   /* index of this call's sample 0 in the pixel's stream */
  uint32_t flags;          /* ZRT_CQ_* */
  uint32_t reserved[5];
} zrt_camera_query;
int zrt_ctx_camera(zrt_ctx* ctx, const zrt_params* params, const zrt_lens* lens, const zrt_camera_query* query,
                   float* dev_sum, float* dev_rgb, void* hip_stream);
/* zrt_ctx_radiance_info's fields of the last camera call (waits for it).  The camera query and
 * the radiance query share one state on a context - rows, parked sums, counters, events - so
 * each info call, and zrt_ctx_debug_radiance, reports the last call of *either* kind:
 * zrt_ctx_camera_info after a later zrt_ctx_radiance answers for that radiance call, and
 * zrt_ctx_radiance_info after a zrt_ctx_camera for the camera call (samples = pixels of the
 * rectangle x n_samples).  ZRT_E_INVALID before the context's first camera call. */
int zrt_ctx_camera_info(zrt_ctx* ctx, zrt_radiance_info* out);
/* One-shot, host pointers: a context, the call, the copies out.  sum (width * height
 * float4) is read first (NULL: zeros; so pixels outside the rectangle come back as they
 * went in) and written back; it, out_rgb (width * height * 3 f32, read first likewise) and
 * info may be NULL. */
int zrt_render_lens(const zrt_scene* scene, const zrt_params* params, const zrt_lens* lens,
                    const zrt_camera_query* query, float* sum, float* out_rgb, zrt_radiance_info* info);

/* How zrt_ctx_camera launches (no device; the launch path calls the same function).  Slots
 * enumerate the rectangle in 8 x 8 tiles anchored at (x0, y0), row-major over the tiles, 64
 * consecutive slots per tile: slot t * 64 + l is pixel (x0 + 8 (t % tiles_w) + (l & 7),
 * y0 + 8 (t / tiles_w) + (l >> 3)), so a wave's primary rays are a tile, as in the render;
 * slots outside the rectangle do no work.  radiance is zrt_debug_radiance_plan's over the
 * slots (n = slots; its key_offset is seed * 0x9E3779B97F4A7C15).  Refuses what
 * zrt_ctx_camera refuses of params and query; zrt_lens_check refuses what it refuses of the
 * lens.  The launch reads ZRT_RADIANCE_PARTIAL_CAP and ZRT_RADIANCE_GRID as the radiance
 * query does. */
typedef struct zrt_camera_plan {
  uint64_t slots;              /* tiles_w x tiles_h x 64 */
  uint64_t pixels;             /* w x h */
  uint32_t tiles_w, tiles_h;
  zrt_radiance_plan radiance;
} zrt_camera_plan;
int zrt_debug_camera_plan(const zrt_params* params, const zrt_camera_query* query, uint32_t cu_count,
                          uint64_t partial_cap_bytes, zrt_camera_plan* out);
int zrt_lens_check(const zrt_lens* lens);

/* A lens of `kind` at a pose (host only), from the very u, v, w and h that zrt_camera_init
 * computes (camera.zig:17-35; viewport_width = aspect * 2 h), in f32, in this order:
 *   horizontal = u * (focus_dist * viewport_width), vertical = v * (focus_dist * viewport_height)
 *   lower_left_corner = ((look_from - horizontal * 0.5f) - vertical * 0.5f) - w * focus_dist
 *   axis_u = u * (aperture * 0.5f), axis_v = v * (aperture * 0.5f)   (pinhole, thin, equirect)
 *   axis_u = u, axis_v = v                                             (ortho, fisheye)
 *   axis_w = -w                                                        (the viewing direction)
 *   half_fov = fisheye_fov_deg * (pi / 360) in f32
 * With focus_dist = 1 the plane equals zrt_camera_init's bit for bit, whatever the aperture.
 * ZRT_E_INVALID: an unknown kind, or a result zrt_lens_check refuses. */
int zrt_lens_init(uint32_t kind, const float look_from[3], const float look_at[3], const float vup[3],
                  float vfov_deg, float aspect, float aperture, float focus_dist, float fisheye_fov_deg,
                  zrt_lens* out);
/* The lens of `kind` at the pose of a zrt_camera (host only; what the command line's
 * ZRT_LENS uses), in f32 in this order: c = ((lower_left_corner + horizontal * 0.5f) +
 * vertical * 0.5f) - origin, D = |c| = sqrtf((c.x c.x + c.y c.y) + c.z c.z), the viewing
 * direction f = c * (1.0f / D), u = horizontal * (1.0f / |horizontal|), v = vertical *
 * (1.0f / |vertical|).
 * focus_dist <= 0: the camera's own plane, unchanged (a pinhole is then the camera bit for
 * bit); else horizontal and vertical scaled by focus_dist / D and lower_left_corner =
 * ((origin - horizontal * 0.5f) - vertical * 0.5f) + f * focus_dist.  axis_u, axis_v and
 * half_fov as zrt_lens_init; axis_w = f. */
int zrt_lens_from_camera(uint32_t kind, const zrt_camera* camera, float aperture, float focus_dist,
                         float fisheye_fov_deg, zrt_lens* out);

/* ---- denoising lens frames: lens features, moments, filters on a rectangle ------- *
 * What makes a low-sample camera-query frame usable: first-hit features along the lens
 * model's centre rays, the second moment of the query's chunk sums (and the variance
 * plane it gives), and both filters over a pixel rectangle instead of raytrace.zig:168's
 * square.  All arithmetic is f32, nothing fused, IEEE `/` and sqrtf, in the order written.
 * A zrt_rect is a camera query's rectangle: inside the width x height frame, not empty. */
typedef struct zrt_rect { uint32_t x0, y0, w, h; } zrt_rect;

/* Host only; every launch path below calls it.  ZRT_E_INVALID: a null pointer, an empty
 * rectangle, one that leaves the frame, params the camera query would refuse (width or
 * height outside 1 .. 65535, and what every entry point refuses of params). */
int zrt_rect_check(const zrt_params* params, const zrt_rect* rect);

/* zrt_ctx_features along lens rays: the feature buffer (width*height*8 f32, 16-byte aligned,
 * two float4 per pixel, the whole width addressable) of the pixels of rect; pixels outside
 * are not touched.  The centre ray of pixel (x, y): u = float(x) / float(width), v =
 * float(y) / float(height) - the camera query's jitter formula at r1 = r2 = 0.5, exactly -
 * (o, tgt) = model(u, v) as the camera query defines the five models, the thin lens taken at
 * its centre (o = origin, no lens stream drawn), dir = tgt - o, Ray.init.  The hit and the
 * eight floats are zrt_ctx_features': the closest hit in (0.001, inf) through
 * params->traversal with the grazing-triangle guard on; {N, t}, {A, id}; a miss gives N = 0,
 * t = 0, A = backgroundColor(d), id = 0.  With zrt_lens_from_camera(PINHOLE, cam) and rect =
 * {0, 0, height, height} the rectangle equals zrt_ctx_features' bit for bit.
 * It is a query (see "ray queries"): the query's rows, error flag, completion and events, one
 * query in flight per context; after a traversal stack overflow the rectangle's floats are
 * NaN and zrt_ctx_sync reports ZRT_E_UNSUPPORTED once.  Lanes take the rectangle in 8 x 8
 * tiles anchored at (x0, y0), as the camera query's slots.  ZRT_E_INVALID: what
 * zrt_rect_check and zrt_lens_check refuse, a null or misaligned pointer, params that do not
 * fit the context. */
int zrt_ctx_camera_features(zrt_ctx* ctx, const zrt_params* params, const zrt_lens* lens, const zrt_rect* rect,
                            float* dev_features, void* hip_stream);

/* zrt_ctx_camera whose sum.w holds Q, zrt_ctx_accum_variance's second moment: per chunk of
 * the call, in chunk order, l_j = (S_j.r + S_j.g) + S_j.b, Q = Q + l_j * l_j; a ragged last
 * chunk goes into the sums but not into Q.  Q starts at 0, or at the caller's sum.w under
 * ZRT_CQ_ACCUMULATE, so calls over [0, 8) and [8, 16) equal one over [0, 16), Q included,
 * whatever the rounds.  After a device error Q is NaN, as the sums are.  Everything else -
 * sums, means, counters, rounds, refusals, zrt_ctx_camera_info - is zrt_ctx_camera's, which
 * itself keeps writing 0 into sum.w. */
int zrt_ctx_camera_moments(zrt_ctx* ctx, const zrt_params* params, const zrt_lens* lens,
                           const zrt_camera_query* query, float* dev_sum, float* dev_rgb, void* hip_stream);

/* The variance plane of such sums over rect: dev_sum as zrt_ctx_camera_moments left it after
 * n_total samples per pixel, dev_variance width*height f32 in the frame's layout (the plane
 * zrt_ctx_denoise_guided takes).  (k, ik, sc) = zrt_debug_variance_plan(params, n_total),
 * with its refusals (n_total % c != 0, k < 2).  Per pixel of rect: M = (sum.r + sum.g) +
 * sum.b, mean = M * ik, v = Q * ik - mean * mean, v = v > 0 ? v : 0 (a NaN stays NaN), var =
 * v * sc.  Pixels outside rect are not touched.  Elementwise and stateless: not a query;
 * asynchronous on hip_stream (NULL: the context's own). */
int zrt_ctx_camera_variance(zrt_ctx* ctx, const zrt_params* params, const zrt_rect* rect, uint32_t n_total,
                            const float* dev_sum, float* dev_variance, void* hip_stream);

/* Both filters with D = rect.  dev_variance == NULL: the definition of "denoising" (flags
 * must be 0 and dev_out_variance NULL); otherwise that of "variance-guided denoising", with
 * ZRT_DN_DEMODULATE allowed.  Each holds word for word with D = the pixels of rect: a tap
 * outside rect is skipped even though the frame holds valid pixels there, the guided 3 x 3
 * smoothing takes V(p) for a neighbour outside rect, and pixels outside rect are copied,
 * frame and variance, over the whole width x height frame.  height > width is not refused.
 * With rect = {0, 0, height, height} the outputs are zrt_ctx_denoise's and
 * zrt_ctx_denoise_guided's bit for bit.  Buffers as theirs; the context's ping-pong planes
 * and zrt_ctx_denoise_ms serve it as they serve them.  ZRT_E_INVALID: what zrt_rect_check
 * refuses, what they refuse of dn, flags and pointers. */
int zrt_ctx_denoise_rect(zrt_ctx* ctx, const zrt_params* params, const zrt_denoise* dn, uint32_t flags,
                         const zrt_rect* rect, const float* dev_frame, const float* dev_features,
                         const float* dev_variance, float* dev_out, float* dev_out_variance, void* hip_stream);

/* One-shot on one GPU (params->device): a context, zrt_ctx_camera_moments (guided != 0) or
 * zrt_ctx_camera (guided == 0) over the query, zrt_ctx_camera_features,
 * zrt_ctx_camera_variance at n_total = n_samples (guided) and zrt_ctx_denoise_rect over
 * the query's rectangle, then the copies out.  Every device buffer starts zeroed: pixels
 * outside the rectangle come back 0.  dn NULL: zrt_denoise_guided_defaults' filter (guided)
 * or zrt_denoise_defaults'; flags are the caller's and must be 0 when guided == 0.  out_rgb
 * (width*height*3 f32): the filtered frame; out_noisy (may be NULL): the unfiltered frame,
 * bit for bit zrt_render_lens'; out_features (may be NULL): width*height*8 f32; out_variance
 * (may be NULL; guided): width*height f32; info, denoise_ms may be NULL.  ZRT_E_INVALID before
 * any device work: what the calls above refuse of their arguments, and, guided, what the
 * variance plan refuses of n_samples (the sums start zeroed, so they hold the call's samples
 * whatever first_sample and ZRT_CQ_ACCUMULATE say). */
int zrt_render_lens_denoised(const zrt_scene* scene, const zrt_params* params, const zrt_lens* lens,
                             const zrt_camera_query* query, const zrt_denoise* dn, uint32_t guided, uint32_t flags,
                             float* out_rgb, float* out_noisy, float* out_features, float* out_variance,
                             zrt_radiance_info* info, double* denoise_ms);

/* ---- host-side scene ingestion (the caller side of the seam) ------------- *
 * Restatement of scenes.zig / obj_reader.zig / png_image.zig texture loading
 * so tests and bench can build the reference's scenes without Zig.  Assets are
 * read from `assets_dir` (OBJ files and P6 PPM textures, tools/prepare_assets.py). */
typedef struct zrt_scene_data zrt_scene_data;

/* Build scene `scene_index` as scenes.zig:267-277 does (0 man+ball, 1 seven
 * spheres, 2 bunny+ball, 3 teapot+ball, 4 teapot+ball circle, 5 goat - needs
 * high_poly_goat.obj, which the reference does not ship: ZRT_E_IO without it),
 * plus 6: the textured, subdivided teapot that stands in for config C5
 * (DESIGN.md section 4).  The camera is returned in *camera; the scene view
 * stays valid until zrt_scene_free.  Unknown index -> ZRT_E_INVALID
 * (SceneError.UnkownSceneIndex). */
int zrt_scene_load(uint32_t scene_index, const char* assets_dir,
                   zrt_scene_data** out, zrt_camera* camera);
const zrt_scene* zrt_scene_view(const zrt_scene_data* data);
void zrt_scene_free(zrt_scene_data* data);

/* Binary scene files: a loaded (or any caller-built) scene and its camera
 * written as the flat arrays above, so a million-triangle mesh (the C5
 * substitute: 1.6 M triangles) is read back in a fraction of the OBJ parse +
 * subdivision time.  zrt_scene_read returns the same opaque handle as
 * zrt_scene_load (zrt_scene_view / zrt_scene_free).  ZRT_E_IO on an
 * unopenable / truncated file, ZRT_E_PARSE on a foreign or inconsistent one. */
int zrt_scene_write(const zrt_scene* scene, const zrt_camera* camera, const char* path);
int zrt_scene_read(const char* path, zrt_scene_data** out, zrt_camera* camera);

/* Parse an OBJ file into triangles (obj_reader.zig:114-198), all with material
 * `material`.  *out_prims is malloc'd; free with zrt_free. */
int zrt_obj_read(const char* path, uint32_t material, zrt_prim** out_prims, uint32_t* n_prims);
void zrt_free(void* p);

/* ---- image output (the caller side: main.zig:33 writes the rendered image) -- *
 * `rgb` is a framebuffer as zrt_render returns it (row 0 = bottom).
 * PNG: png_image.zig:96-148 - 8-bit RGB, top row first,
 *      u8(std.math.clamp(255.999 * c, 0, 255)) per channel.
 * PPM: ppm_image.zig - plain P3 text, u32(c * 255.999) clamped to [0, 255].
 * Unopenable path -> ZRT_E_IO (PngError.FailedToOpenFile). */
/* png_image.readFile (png_image.zig:19-94): an 8-bit RGB or RGBA PNG (other
 * color types and depths: ZRT_E_UNSUPPORTED, the reference's
 * UnsupportedPngFeature) as width*height RGB f32, row 0 = bottom, c/255, alpha
 * dropped.  Also reads 8-bit binary PPM (P6).  *out_pixels: free with zrt_free. */
int zrt_image_read_png(const char* path, uint32_t* width, uint32_t* height, float** out_pixels);
int zrt_image_write_png(const char* path, const float* rgb, uint32_t width, uint32_t height);
int zrt_image_write_ppm(const char* path, const float* rgb, uint32_t width, uint32_t height);

/* ---- BVH export (parity of bvh.zig:62-185 against the oracle) ------------- *
 * Node i: box min/max and two children.  A child c >= 0 is a node index; a
 * child c < 0 is primitive (-c - 1) in reference list order.  Leaves are
 * exactly the reference's (one prim on both sides, or s[1], s[0]).  The root
 * is node 0; nodes are in depth-first (left-first) pre-order. */
typedef struct zrt_bvh_node {
  zrt_vec3 min;
  int32_t left;
  zrt_vec3 max;
  int32_t right;
} zrt_bvh_node;

int zrt_bvh_build(const zrt_scene* scene, zrt_bvh_node** out_nodes,
                  uint32_t* n_nodes, uint32_t* max_depth);

/* The same tree built on GPU `device` (bvh.zig:62-185 level by level: each
 * level's stable axis sorts as segmented radix sorts, the split scores as
 * one wave per segment).  Node for node equal to zrt_bvh_build.
 * The context entry points use it for scenes of >= 65536 primitives.
 * ZRT_E_UNSUPPORTED for < 3 primitives or NaN midpoints (the host build
 * handles those). */
int zrt_bvh_build_device(const zrt_scene* scene, uint32_t device, zrt_bvh_node** out_nodes,
                         uint32_t* n_nodes, uint32_t* max_depth);

/* ---- device parity probes ------------------------------------------------ *
 * Evaluate the kernel's own device functions on inputs, for bit-exact
 * comparison with the oracle's restatements:
 *   fn 0 sin, 1 cos (std.math, Go/Cephes), 2 acos, 3 atan (musl), 4 sqrt,
 *   5 atan2(x[i], y[i]), 6 pow(x[i], 5.0), 7 x[i] / y[i] (HIP's IEEE `/`),
 *   8 1 / x[i] and 9 x[i] / y[i] through the kernel's short correctly rounded
 *   sequences (rcp_rn / div_rn, device_math.hpp).
 * zrt_debug_rng writes n outputs of DefaultPrng.init(key).next() computed on
 * the device.  zrt_debug_division runs the device self-check of those short
 * sequences against IEEE `/` and sqrtf (counts[5]: mismatches of the reciprocal
 * and the square root over all 2^32 inputs, of division, unit(), 1/d and the jitter quotient over n hashed
 * inputs each; all zero on a correct build).  All run on `device` and synchronise. */
int zrt_debug_math(int fn, const float* x, const float* y, float* out, uint32_t n, uint32_t device);
int zrt_debug_rng(uint32_t prng, uint64_t key, uint64_t* out, uint32_t n, uint32_t device);
int zrt_debug_division(uint64_t n, uint64_t* counts, uint32_t device);
/* One launch of the adaptive run's compaction (compact_kernel) on its own: the
 * entries of list (n of them, each < n_tiles) whose tile_done word (n_tiles words:
 * samples per pixel, bit 31 set once frozen, as resolve_kernel leaves them) has bit
 * 31 clear, packed in list order.  out (n entries) is uploaded as the output
 * buffer's initial content and copied back after the launch, so entries past
 * *count keep what the caller put there; *count: the entries written.
 * ZRT_E_INVALID: a null pointer, n == 0, or a list entry >= n_tiles (checked on
 * the host: the kernel indexes tile_done with the entries). */
int zrt_debug_compact(const uint32_t* list, uint32_t n, const uint32_t* tile_done, uint32_t n_tiles,
                      uint32_t* out, uint32_t* count, uint32_t device);
/* Host-side check of the kernels' LDS layouts for this scene (no device
 * needed): the scene is flattened as zrt_ctx_create does, then every plan the
 * launch code can make - each sampling loop, stack width, PRNG and a range of
 * max depths - is checked region by region (stack rows, top wide nodes, pool
 * queues, lane state, attenuation rows, materials: in the block's LDS, disjoint,
 * float4 regions 16-B aligned; the lockstep loop's plan within its 6-block
 * share), the FAST loops' 16-bit plans also with their LDS stack rows capped at
 * 1, 2 and 4 (as ZRT_STACK_LDS_ROWS16 caps them).  n_checked: the number of plans
 * checked.  ZRT_E_UNSUPPORTED names the first violation. */
int zrt_debug_lds_plans(const zrt_scene* scene, uint32_t* n_checked);
/* Host-side check of the global buffers the launches of a FAST frame share (no
 * device needed): for every sampling loop, stack width, PRNG, node format, a
 * range of max depths and grid sizes, zrt_render's sizing of the attenuation
 * rows and stack overflow rows (the render launch's need, grown to its
 * scheduling probe's) is checked against what each of the two launches needs
 * (zrt::buffer_need; the same check guards every launch, ZRT_E_UNSUPPORTED
 * instead of a device fault).  legacy = 1 applies the sizing before the round-5
 * fix (the probe shared the render's attenuation rows without growing them):
 * it must fail where a loop keeps more rows in LDS than the probe's 4.
 * The 16-bit stacks are checked with their LDS rows capped at 1, 2 and 4 too.
 * n_checked: configurations checked. */
int zrt_debug_buffer_plans(const zrt_scene* scene, uint32_t legacy, uint32_t* n_checked);
/* The launch decision zrt_ctx_render_tiles would take for this scene and these
 * params, with no device: the scene is flattened as zrt_ctx_create does, then
 * the function the render path itself calls decides the sampling loop, the stack
 * width and the block's LDS plan, under the same environment knobs (ZRT_WF,
 * ZRT_POOL, ZRT_LIST_LANES, ZRT_QNODES, ZRT_ATT_LDS_ROWS, ZRT_STACK_LDS_ROWS,
 * ZRT_STACK_LDS_ROWS16, ...).  Only max_depth, traversal, prng, flags and
 * bounded_volume_hierarchy of the params are read (tests only). */
typedef struct zrt_launch_plan {
  uint32_t mode;               /* 0 list, 1 BINARY, 2 REFERENCE, 3 FAST */
  uint32_t kmode;              /* the kernel's loop: mode, or 4 wavefront, 5 / 7 (guarded) path pool,
                                  8 / 9 (guarded) path pool over compressed nodes, 6 list with per-lane items */
  uint32_t sampling_loop;      /* what zrt_stats.sampling_loop reports for it (7, 8, 9 -> 5) */
  uint32_t stk16;              /* 16-bit stack entries (else 32-bit) */
  uint32_t wf, pool, qnodes, guard_on;
  uint32_t stack_depth;        /* stack rows the traversal may use */
  uint32_t stack_rows;         /* of them in LDS; the rest are global overflow rows */
  uint32_t att_rows;           /* attenuation rows in LDS */
  uint32_t att_rows_per_path;  /* global attenuation rows allocated per path (lane) */
  uint32_t mats_in_lds;        /* the material table has a region in the plan */
  uint32_t lds_bytes;          /* the block's dynamic LDS */
  uint64_t ovf_bytes_per_lane; /* global stack overflow rows allocated per lane, in bytes */
} zrt_launch_plan;
int zrt_debug_launch_plan(const zrt_scene* scene, const zrt_params* params, zrt_launch_plan* out);
/* Whether zrt_ctx_render_tiles would launch the lean kernel for this scene, camera
 * and params, with no device (decided by the functions the render path calls).
 * The lean kernel is the timed lockstep FAST kernel compiled without image
 * textures, dielectrics, the ray-origin check, the IEEE 1/det fallback and the
 * scanline rows.  *lean is 1 only when all of this holds: the launch plan's loop is
 * the lockstep FAST loop with max_depth >= 1 and the material table in LDS; the
 * scene has no dielectric and no image-textured material and every triangle is under
 * the fast 1/det bound; ZRT_FLAG_SCANLINES and ZRT_FLAG_STATS are clear; the camera
 * lies inside the scene's ray-origin bound; the environment does not say ZRT_LEAN=0.
 * (tests only) */
int zrt_debug_lean_kernel(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
                          uint32_t* lean);
/* Host-side check of the compressed wide nodes built for this scene (no device
 * needed): every plane of every node's eight octant copies decodes exactly to
 * an f32, every slot's decoded box contains the full node's box of that slot,
 * near / far bytes are the full node's min / max in the octant's order, and
 * every leaf slot's record holds the full node's leaf box and primitive refs bit
 * for bit.  n_checked: the slots checked.  ZRT_E_UNSUPPORTED names the first
 * violation (or a tree the encoder refused). */
int zrt_debug_qnodes(const zrt_scene* scene, uint64_t* n_checked);
/* The size check context creation makes on a flattened wide tree (no device
 * needed): a ray's octant copy lies oct * stride_f4 float4s into the nodes and
 * oct * n_top * node_f4 into the top levels in LDS, and the kernels form both
 * products from the factors' low 24 bits.  ZRT_E_UNSUPPORTED when stride_f4 or
 * n_top * node_f4 reaches 2^24 (zrt_ctx_create returns the same for such a scene),
 * ZRT_OK otherwise - and always for a library built with ZRT_OCT_MUL24=0.
 * (tests only) */
int zrt_debug_octant_offsets(uint32_t stride_f4, uint32_t n_top, uint32_t node_f4);
/* The class of each of this rank's tiles as zrt_ctx_render_tiles would split them,
 * with no device: classes[lt] for local tile lt (at most cap words are written), 0
 * for a general tile, ZRT_TILE_SKY for a tile no primary ray of which can return a
 * hit from the reference's closest-hit query, whatever the jitter, the seed, the
 * sample count or the generator (such tiles render in a kernel without traversal;
 * the frame is the same bit for bit).  Every tile is general unless the launch is the
 * lockstep FAST loop with max_depth >= 1, without ZRT_FLAG_SCANLINES and
 * ZRT_FLAG_GUARD, from a camera inside the scene's ray-origin bound, over a scene
 * with no non-finite plane; and when the environment says ZRT_SKY_TILES=0.
 * ZRT_TILE_ONE_SPHERE | s for a tile no primary ray of which can return a hit from any
 * primitive but the sphere in device primitive slot s (a ray of the tile may hit s or
 * nothing); every one-sphere tile of a call carries the same s.  Only where, besides
 * the conditions above, the launch is lean-eligible (zrt_debug_lean_kernel's conditions
 * but for ZRT_FLAG_STATS), the sphere's leaf is a child of the wide tree's root, and the
 * environment does not say ZRT_SPHERE_TILES=0.  Test (word & ZRT_TILE_SKY) == 0 &&
 * (word & ZRT_TILE_ONE_SPHERE) != 0.
 * margins (4 doubles, or NULL): the largest distance past a sphere's surface and past
 * a triangle at which the classifier still counts a ray as a possible hit, and the
 * triangles' two coefficients (reach = k_ao |ao| + k_c).  n_sky: the rank's sky tiles.
 * zrt_ctx_debug_counters slot 47 of a context's last launch holds the same count,
 * slot 46 the tiles it rendered as one-sphere.
 * (tests only) */
#define ZRT_TILE_SKY 0x80000000u
#define ZRT_TILE_ONE_SPHERE 0x40000000u
int zrt_debug_tile_classes(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
                           uint32_t* classes, uint32_t cap, uint32_t* n_tiles, uint32_t* n_sky, double* margins);
/* The list index (zrt_scene::prims) of the primitive in each device primitive slot, as
 * zrt_ctx_create flattens the scene under these params, with no device: prims[slot] for
 * slot < *n_slots (at most cap words are written).  The slot in a ZRT_TILE_ONE_SPHERE class
 * word is such a slot.  (tests only) */
int zrt_debug_slot_prims(const zrt_scene* scene, const zrt_params* params, uint32_t* prims, uint32_t cap,
                         uint32_t* n_slots);

#ifdef __cplusplus
}
#endif
#endif /* ZRT_H */
