/*
 * hrt.h — the drop-in C ABI of the MI355X path-tracing inner loop (libhrt.so).
 *
 * What it replaces (reference = SkillerRaptor/hyper-ray-tracer, a Rust crate with no FFI of its own):
 *   - the trait surface the scene builders construct (src/hittable/mod.rs:19-25 `Hittable`,
 *     src/materials/mod.rs:15-19 `Material`, src/textures/mod.rs:14-16 `Texture`): a GPU cannot call
 *     back into trait objects per ray, so each concrete type gets a constructor here that records a
 *     lowered description (the additive `lower()` a Rust binding adds to each type);
 *   - `Application::render` (src/application.rs:393-475) + `ray_color` (:477-495): the per-tile,
 *     per-pixel, per-sample loop, which becomes hrt_render / hrt_render_tiles_device (one persistent
 *     HIP megakernel launch for a whole tile set);
 *   - `Camera::new`/`resize` (src/camera.rs:34-83): hrt_camera_init.
 *
 * Conventions
 *   - Every function returns hrt_status (0 = OK) and never unwinds; the reference's panics (empty BVH
 *     bvh_node.rs:38, NaN bbox bvh_node.rs:31/76, missing image image_texture.rs:20, gen_range with
 *     lo >= hi) become status codes.  hrt_last_error() returns a thread-local message.
 *   - Ids returned through uint32_t* are indices into the scene's texture / material / node tables.
 *     Inputs (Perlin tables, image bytes, child lists) are deep-copied during the call.
 *   - A scene is mutable until hrt_scene_commit, immutable afterwards; rendering is re-entrant per
 *     scene (each call uses its own stream-ordered scratch).
 *   - Image layout: pixel (x, y) with y = 0 the BOTTOM row (src/application.rs:444-445); output of a
 *     w*h region is RGBA f32 at index (x-x0) + w*(y-y0), alpha = 1 (src/application.rs:451-456).
 */
#ifndef HRT_HRT_H
#define HRT_HRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t hrt_status;
enum {
  HRT_OK = 0,
  HRT_ERR_INVALID_ARG = 1, /* bad id, null pointer, bad enum, lo >= hi ... */
  HRT_ERR_EMPTY = 2,       /* BvhNode::new with no objects (bvh_node.rs:38) */
  HRT_ERR_NO_BBOX = 3,     /* object without bounding box inside a BVH (bvh_node.rs:42,79) */
  HRT_ERR_NAN = 4,         /* NaN in a bounding box / sort key (bvh_node.rs:31,76) */
  HRT_ERR_STATE = 5,       /* mutation after commit, render before commit, ... */
  HRT_ERR_HIP = 6,         /* HIP runtime error (message in hrt_last_error) */
  HRT_ERR_OOM = 7,
  HRT_ERR_UNSUPPORTED = 8  /* e.g. a ConstantMedium nested inside another medium's boundary */
};

typedef struct hrt_scene hrt_scene;

/* rect.rs:12-17 */
enum { HRT_PLANE_XY = 0, HRT_PLANE_YZ = 1, HRT_PLANE_ZX = 2 };
/* rotation.rs:10-25 */
enum { HRT_AXIS_X = 0, HRT_AXIS_Y = 1, HRT_AXIS_Z = 2 };

/* Camera after Camera::resize (src/camera.rs:16-31, 67-83). */
typedef struct hrt_camera {
  float origin[3];
  float lower_left_corner[3];
  float horizontal[3];
  float vertical[3];
  float u[3], v[3], w[3];
  float lens_radius;
  float time0, time1;
} hrt_camera;

/* Render knobs: src/arguments.rs:23-47 (width/height/samples/depth/tile) + the values the reference
 * hard-codes (background per scene application.rs:132-197, t_min = 0.001 at :482) + the seed that
 * replaces thread_rng.  Pixels are keyed by their index in the FULL width x height image. */
typedef struct hrt_render_params {
  uint32_t width, height;   /* full image (u = (x+xi)/(width-1), application.rs:444); each must lie in
                               [2, 65535] (HRT_ERR_INVALID_ARG otherwise): the camera divisions are
                               computed with host reciprocals proven exact on that range only */
  uint32_t samples;         /* spp (application.rs:443) */
  uint32_t max_depth;       /* ray_color depth (application.rs:478); reference CLI default 10 */
  uint32_t sample_offset;   /* first sample index (0; >0 splits one pixel's samples across jobs) */
  uint32_t flags;           /* HRT_RENDER_* bits */
  float t_min;              /* 0.001 */
  float background[3];
  uint64_t seed;
} hrt_render_params;

/* hrt_render_params.flags */
enum {
  HRT_RENDER_COUNT_WORK = 1, /* instrumented kernel: stats also count node visits / prim tests / texture
                                evaluations (for the algorithmic-bytes model; slower) */
  HRT_RENDER_NO_LDS = 2,     /* keep the scene in global memory even when it fits in LDS (A/B) */
  HRT_RENDER_REFERENCE_CULL = 8, /* aabb.rs's per-axis box test alone (the verbatim reference traversal) */
  HRT_RENDER_FAST_CULL = 16,     /* APPROXIMATE: plain slab culling; differs from the reference on ~1e-7 of
                                    rays (f32 grazing hits the reference accepts outside a box).  Ignored where a
                                    bounding box does not hold its geometry (a ZX rect whose two extents differ:
                                    rect.rs:97-102) and for a shutter outside the boxes' interval */
  HRT_RENDER_SAH = 32            /* APPROXIMATE, with FAST_CULL on sphere-only scenes: SAH octant streams
                                    (traversal order changes which of two near-equal f32 hits wins) */
};

/* hrt_image_write formats (the reference only displays its frame) */
enum {
  HRT_IMAGE_PFM = 0, /* float RGB, little-endian, rows bottom to top: the frame bit for bit */
  HRT_IMAGE_PPM = 1  /* 8-bit binary RGB, rows top to bottom, 256 * clamp(c, 0, 0.999) per channel */
};

typedef struct hrt_tile {
  uint32_t x, y, w, h; /* image coordinates, y up */
} hrt_tile;

/* Work counters of one render call (exact, counted on the device). */
typedef struct hrt_render_stats {
  uint64_t segments;        /* world.hit calls == rays (application.rs:482) */
  uint64_t samples;         /* primary samples = pixels * spp */
  uint64_t pixels;
  uint64_t node_visits;     /* HRT_RENDER_COUNT_WORK only: node-stream entries read */
  uint64_t prim_tests;      /* HRT_RENDER_COUNT_WORK only: primitive intersection tests */
  uint64_t tex_evals;       /* HRT_RENDER_COUNT_WORK only: Texture::value evaluations */
  uint64_t walk_slots;      /* HRT_RENDER_COUNT_WORK only: 64 x wave iterations of the node walk
                               (node_visits / walk_slots = SIMD lane utilisation of the walk) */
  uint64_t shade_slots;     /* HRT_RENDER_COUNT_WORK only: 64 x wave passes through shading */
  uint64_t prim_slots;      /* HRT_RENDER_COUNT_WORK only: 64 x wave runs of the batched leaf-test block
                               (walk kernels; 0 for the segment kernels) */
  uint64_t phase_cycles[3]; /* HRT_RENDER_COUNT_WORK, walk kernels: shader cycles summed over
                               waves spent in [0] work claim + sample start, [1] walk, [2] shading */
  uint64_t park_slots;      /* HRT_RENDER_COUNT_WORK, walk kernels: lane slots of walk steps spent parked on
                               a leaf (waiting for the batched primitive test) */
  uint64_t wait_slots;      /* ... spent with the walk done, waiting for the wave to leave the walk and shade */
  uint64_t leaf_cycles;     /* HRT_RENDER_COUNT_WORK, walk kernels: the part of phase_cycles[1] spent in the batched
                               leaf tests (sphere tests / leaf programs) */
  uint64_t walk_steps;      /* HRT_RENDER_COUNT_WORK, walk kernels: lane slots of the walk loop that stepped a node
                               (walk_steps / walk_slots = the walk's SIMD lane utilisation; node_visits also counts
                               the nodes leaf programs test) */
} hrt_render_stats;

/* Scene description of one reference preset (application.rs:132-211). */
typedef struct hrt_preset_info {
  float look_from[3];
  float look_at[3];
  float fov;
  float aperture;
  float focus_dist;
  float time0, time1;
  float background[3];
  uint32_t root;
} hrt_preset_info;

/* Reference scenes (src/arguments.rs:9-19) + build-defined benchmark scenes. */
enum {
  HRT_PRESET_RANDOM = 0,             /* application.rs:497-565 (BASELINE configs 1, 2) */
  HRT_PRESET_TWO_SPHERES = 1,        /* :567-587 */
  HRT_PRESET_TWO_PERLIN_SPHERES = 2, /* :589-602 */
  HRT_PRESET_EARTH = 3,              /* :604-612 */
  HRT_PRESET_SIMPLE_LIGHT = 4,       /* :614-637 */
  HRT_PRESET_CORNELL = 5,            /* :639-721 (config 5) */
  HRT_PRESET_CORNELL_SMOKE = 6,      /* :723-815 */
  HRT_PRESET_FINAL = 7,              /* :817-935 */
  HRT_PRESET_EARTH_PERLIN = 8,       /* config 3: earth (0,2,0) r2 over the Perlin ground of :589-602 */
  HRT_PRESET_RANDOM_10K = 9,         /* config 4: :511-545 with a, b in [-50, 50) */
  HRT_PRESET_FEATURES = 10,          /* X/Z rotations, lists, nested instances, media in instances */
  HRT_PRESET_RANDOM_40K = 11,        /* :511-545 with a, b in [-100, 100): 39.9k leaves, so the walk stream's
                                        hierarchy is built on the device by default */
  HRT_PRESET_MOTION = 12,            /* moving spheres with their own shutter intervals (moving_sphere.rs:53-58
                                        per sphere: no scene-wide motion factor), a sphere-kernel scene */
  HRT_PRESET_COUNT = 13
};

const char* hrt_last_error(void);
const char* hrt_version(void);
/* ABI version.  Structs the library writes (hrt_render_stats, hrt_launch_info, hrt_blob_info) have
 * grown between releases with no size field, so a caller built against an older header would be written past
 * its buffers: check hrt_abi_version() == HRT_ABI_VERSION once before any other call, and rebuild on a mismatch.
 *   6: hrt_abi_version; hrt_launch_info.knobs is the launch's snapshot, commit-time knobs as "commit:NAME=value"
 *   5: hrt_launch_info.knobs (+256 B), hrt_render_stats.walk_steps, hrt_blob_info walk_c16/walk_nodes/walk_pbase,
 *      hrt_scene_options, hrt_scene_set_view, hrt_debug_sample_chunks */
#define HRT_ABI_VERSION 6u
uint32_t hrt_abi_version(void);

/* ---- scene lifetime ---- */
hrt_status hrt_scene_create(hrt_scene** out);
void hrt_scene_destroy(hrt_scene* scene);

/* ---- textures (src/textures/) ---- */
hrt_status hrt_tex_solid(hrt_scene* s, float r, float g, float b, uint32_t* id);
hrt_status hrt_tex_checker(hrt_scene* s, uint32_t odd, uint32_t even, uint32_t* id);
/* ranvec: 256*3 f32 unit vectors; perm: 3*256 u32 (x, y, z permutations), perlin_noise.rs:14-19 */
hrt_status hrt_tex_noise(hrt_scene* s, float scale, const float* ranvec, const uint32_t* perm,
                         uint32_t* id);
/* Decoded image bytes (image_texture.rs:19-33); data may be NULL/empty -> magenta (:37-39). */
hrt_status hrt_tex_image(hrt_scene* s, const uint8_t* data, uint32_t width, uint32_t height,
                         uint32_t components, uint32_t* id);

/* ---- materials (src/materials/) ---- */
hrt_status hrt_mat_lambertian(hrt_scene* s, uint32_t albedo_tex, uint32_t* id);
hrt_status hrt_mat_metal(hrt_scene* s, float r, float g, float b, float fuzz, uint32_t* id);
hrt_status hrt_mat_dielectric(hrt_scene* s, float index_of_refraction, uint32_t* id);
hrt_status hrt_mat_diffuse_light(hrt_scene* s, uint32_t emit_tex, uint32_t* id);
hrt_status hrt_mat_isotropic(hrt_scene* s, uint32_t albedo_tex, uint32_t* id);

/* ---- hittables (src/hittable/) ---- */
hrt_status hrt_node_sphere(hrt_scene* s, const float center[3], float radius, uint32_t mat,
                           uint32_t* id);
hrt_status hrt_node_moving_sphere(hrt_scene* s, const float center0[3], const float center1[3],
                                  float time0, float time1, float radius, uint32_t mat,
                                  uint32_t* id);
hrt_status hrt_node_rect(hrt_scene* s, int32_t plane, float a0, float a1, float b0, float b1,
                         float k, uint32_t mat, uint32_t* id);
hrt_status hrt_node_cuboid(hrt_scene* s, const float box_min[3], const float box_max[3],
                           uint32_t mat, uint32_t* id);
hrt_status hrt_node_translate(hrt_scene* s, uint32_t child, const float displacement[3],
                              uint32_t* id);
hrt_status hrt_node_rotate(hrt_scene* s, int32_t axis, uint32_t child, float angle_degrees,
                           uint32_t* id);
/* The medium's isotropic phase texture is given as a texture id (constant_medium.rs:22-29). */
hrt_status hrt_node_constant_medium(hrt_scene* s, uint32_t boundary, float density,
                                    uint32_t albedo_tex, uint32_t* id);
hrt_status hrt_node_list(hrt_scene* s, const uint32_t* children, uint32_t n, uint32_t* id);
/* BvhNode::new(objects, t0, t1) (bvh_node.rs:27-63): built immediately, consumes the children. */
hrt_status hrt_node_bvh(hrt_scene* s, const uint32_t* children, uint32_t n, float time0,
                        float time1, uint32_t* id);
/* Hittable::count (hittable/mod.rs:24) and bounding_box (:22). has_box = 0 when None. */
hrt_status hrt_node_count(const hrt_scene* s, uint32_t node, uint32_t* count);
hrt_status hrt_node_bounding_box(const hrt_scene* s, uint32_t node, float time0, float time1,
                                 int32_t* has_box, float box_min[3], float box_max[3]);

/* Scene options: explicit configuration, as the reference takes its configuration as arguments
 * (src/arguments.rs:23-47); the library reads nothing that can change an image from the environment.
 * All-zero is the default.  Set before the nodes they affect (bvh_ties: hrt_node_bvh and the preset
 * builders; everything else: hrt_scene_commit and the renders); after commit, HRT_ERR_STATE. */
typedef struct hrt_scene_options {
  uint32_t bvh_ties;       /* 0: BvhNode::new's equal sort keys in stable order; 1: each run of ties reversed
                              (another order Rust's sort_unstable_by may produce, bvh_node.rs:34) */
  uint32_t walk_tree;      /* 0: the walk's hierarchy re-grouped over the reference leaf order; 1: the reference
                              BvhNode tree itself (same image bit for bit) */
  uint32_t chunk_min;      /* sample chunks (a pixel's samples summed in chunks, then the chunk sums in chunk
                              order): smallest chunk, 0 = the scene class's default */
  uint32_t chunk_max;      /* at most this many head chunks, 0 = default */
  uint32_t chunk_uniform;  /* 1: no halving tail chunks */
} hrt_scene_options;
hrt_status hrt_scene_set_options(hrt_scene* s, const hrt_scene_options* options);
hrt_status hrt_scene_get_options(const hrt_scene* s, hrt_scene_options* options);
/* Placement hint (no reference counterpart; never changes an image's bits): the camera most renders of this
 * scene will use (NULL: none, the default).  A walk stream too large for LDS keeps part of its node parts in
 * LDS and reads the rest from global memory; with a view, hrt_scene_commit stages the node parts that camera
 * rays through a 128 x 128 grid of the view's image plane visit most instead of those
 * under the largest boxes.  Any placement renders the same image bit for bit.  Before commit (HRT_ERR_STATE
 * after). */
hrt_status hrt_scene_set_view(hrt_scene* s, const hrt_camera* view);

hrt_status hrt_scene_set_root(hrt_scene* s, uint32_t node);
/* Flatten + upload to HIP device `device` (-1: the calling thread's current device). */
hrt_status hrt_scene_commit(hrt_scene* s, int32_t device);

/* Reference scene builders (application.rs:497-935) driven by a seeded stream in place of
 * thread_rng.  `image` feeds the Earth texture (earthmap.jpg decoded by the caller, or synthetic). */
hrt_status hrt_preset_build(hrt_scene* s, int32_t preset, uint64_t scene_seed, const uint8_t* image,
                            uint32_t image_w, uint32_t image_h, uint32_t image_c,
                            hrt_preset_info* info);

/* Camera::new + resize (camera.rs:34-83). */
hrt_status hrt_camera_init(hrt_camera* cam, const float look_from[3], const float look_at[3],
                           float fov_degrees, float aperture, float focus_dist, float time0,
                           float time1, int32_t width, int32_t height);

/* ---- rendering ---- */
/* Render `n_tiles` tiles into device memory d_rgba (tiles packed back to back, tile i at
 * 4 * sum_{j<i} w_j*h_j floats; each tile row-major with y up).  Asynchronous on `stream`
 * (a hipStream_t, NULL = default stream).  stats (optional, host pointer) is filled after an
 * internal stream synchronisation when non-NULL.
 * Errors of the launch itself: with stats, HRT_ERR_STATE when the walk watchdog stopped walks that
 * could not end (corrupt scene data; the frame is incomplete).  Without stats the call returns before
 * the kernel ends; such a launch is then reported as HRT_ERR_STATE by the first later call on the
 * scene that finds it finished (the next hrt_render_* call, or hrt_scene_synchronize).  That report belongs to
 * the scene, not to a thread: with several threads on one scene it goes to whichever call sees the launch first,
 * on whatever thread, and to that call alone.
 * Threads: the launches of one scene are issued one at a time (a call holds the scene's launch lock while it
 * enqueues, and a call with stats until its kernel has ended); the kernels of different calls still overlap on
 * their streams.  Results never depend on which other calls are in flight. */
hrt_status hrt_render_tiles_device(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p,
                                   const hrt_tile* tiles, uint32_t n_tiles, float* d_rgba,
                                   void* stream, hrt_render_stats* stats);
/* Wait for every render launched on the scene; HRT_ERR_STATE if one of them did not complete its
 * frame (walk watchdog) and no earlier call has reported it. */
hrt_status hrt_scene_synchronize(hrt_scene* s);
/* One delivered tile (application.rs:45-52 Tile): tile-grid indices (pixel origin = index * tile_size),
 * size in pixels, and RGBA f32 pixels row-major in the tile (row 0 = bottom).  `pixels` is valid only
 * during the callback. */
typedef struct hrt_tile_pixels {
  uint32_t x, y;
  uint32_t width, height;
  const float* pixels;
} hrt_tile_pixels;
typedef void (*hrt_tile_fn)(const hrt_tile_pixels* tile, void* user);
/* Application::render with progressive delivery (application.rs:393-475 + the mpsc receive of
 * :284-306): this rank's tiles of the hrt_tile_grid(width, height, tile_size, rank, world) grid are
 * rendered in launches of `batch` tiles; each finished batch is copied back and passed to `fn` tile by
 * tile (grid order) while the next batch renders.  Pixels are those of hrt_render on the same tile. */
hrt_status hrt_render_progressive(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p,
                                  uint32_t tile_size, uint32_t rank, uint32_t world, uint32_t batch,
                                  hrt_tile_fn fn, void* user, hrt_render_stats* stats);
/* One region into device memory. */
hrt_status hrt_render_device(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p,
                             uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, float* d_rgba,
                             void* stream, hrt_render_stats* stats);
/* One region into caller-owned host memory (w*h*4 floats); synchronous. */
hrt_status hrt_render(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p, uint32_t x0,
                      uint32_t y0, uint32_t w, uint32_t h, float* rgba_out, hrt_render_stats* stats);

/* Reference tile grid (application.rs:363-364, 404-430 with integer ragged edges) and its
 * round-robin split across `world` ranks: writes up to `cap` tiles of rank `rank`; *n = count. */
hrt_status hrt_tile_grid(uint32_t width, uint32_t height, uint32_t tile_size, uint32_t rank,
                         uint32_t world, hrt_tile* tiles, uint32_t cap, uint32_t* n);

/* ---- progressive sample accumulation ---- */
/* A device-resident accumulator of raw per-pixel radiance sums (RGB f32, 16 B per pixel) for a tile set of one
 * frame.  Renders add sample ranges of every pixel into it, and it can be resolved to a displayable frame at any
 * time: refinement pass by pass (a whole frame at 16 spp after a few milliseconds, then more samples), a frame
 * whose samples are split across devices or jobs (download, upload, merge), checkpoint and resume.
 *
 * THE BIT CONTRACT (next to hrt_scene_options.chunk_*, which fixes the bits of one render):
 *   - one hrt_accum_add computes the pass sum of a pixel exactly as hrt_render does for those params: the chunk
 *     schedule of p->samples (hrt_debug_sample_chunks), chunk sums added in chunk order starting from chunk 0's;
 *   - the accumulator then does acc = acc + pass_sum per channel in f32; hrt_accum_merge does dst = dst + src;
 *   - hrt_accum_resolve gives sqrtf(acc * (1.0f / (float)samples)), the render calls' expression.
 * So one add into an empty accumulator followed by a resolve to HRT_ACCUM_F32 equals hrt_render_tiles_device
 * with the same params bit for bit, and a frame of several passes is a function of the PASS SCHEDULE alone (which
 * sample ranges were added or merged, in which order): it never depends on the tile split or the device count.
 *
 * Frame identity: the first add or upload fixes it: the camera's bytes and the params' width, height, max_depth,
 * flags, t_min, background and seed (everything but samples and sample_offset).  A later add, upload or merge with
 * another identity is HRT_ERR_INVALID_ARG; hrt_accum_reset clears it.
 * Sample ranges: the accumulator keeps the sorted, disjoint, coalesced [begin, end) ranges it holds.  An add,
 * upload or merge that overlaps one of them (a sample counted twice biases the image silently) or whose end
 * exceeds 2^32 is HRT_ERR_INVALID_ARG and changes nothing.
 * Streams: as hrt_render_tiles_device: work is asynchronous on `stream`, the caller orders its uses of an
 * accumulator as it does those of d_rgba, and the host bookkeeping (ranges, identity) is updated at call time.
 * hrt_accum_resolve_host, hrt_accum_download and hrt_accum_upload wait for the device.  An add that reports
 * HRT_ERR_STATE with stats (walk watchdog) leaves the accumulator invalid: only reset and destroy then succeed.
 * The accumulator must be destroyed before its scene, and calls on ONE accumulator must not run concurrently
 * (different accumulators of a scene may be used from different threads, as the render calls may). */
typedef struct hrt_accum hrt_accum;
enum {
  HRT_ACCUM_F32 = 0,  /* RGBA f32: sqrt(sum * (1 / samples)), alpha 1: the render calls' rule */
  HRT_ACCUM_RGBA8 = 1 /* 4 x u8: hrt_image_write's PPM rule per channel on the F32 value, alpha 255 */
};
/* Sums for `tiles` of a width x height image, packed as hrt_render_tiles_device packs its output; zeroed, no
 * samples.  The scene must be committed (HRT_ERR_STATE); the accumulator lives on the scene's device. */
hrt_status hrt_accum_create(hrt_scene* s, uint32_t width, uint32_t height, const hrt_tile* tiles, uint32_t n_tiles,
                            hrt_accum** out);
/* hrt_accum_create with flags (0: hrt_accum_create itself) */
enum {
  HRT_ACCUM_NOISE = 1,   /* also keep the noise plane (f32 per pixel) that hrt_accum_noise reads: see below */
  HRT_ACCUM_FEATURES = 4 /* also keep the two first-hit feature planes (2 x 16 B per pixel): see below (2 is not a flag) */
};
hrt_status hrt_accum_create_ex(hrt_scene* s, uint32_t width, uint32_t height, const hrt_tile* tiles, uint32_t n_tiles,
                               uint32_t flags, hrt_accum** out);
void hrt_accum_destroy(hrt_accum* a);
hrt_status hrt_accum_reset(hrt_accum* a, void* stream);
/* Render samples [p->sample_offset, p->sample_offset + p->samples) of every pixel and add them.  stats: the
 * counters of this pass alone (synchronises, as hrt_render_tiles_device). */
hrt_status hrt_accum_add(hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, void* stream,
                         hrt_render_stats* stats);
/* hrt_accum_add, and the frame after this pass resolved to d_out by the same kernel that adds the pass (a
 * preview after every pass costs no extra kernel). */
hrt_status hrt_accum_add_resolve(hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, int32_t format,
                                 void* d_out, void* stream, hrt_render_stats* stats);
hrt_status hrt_accum_samples(const hrt_accum* a, uint64_t* samples);
/* d_out: device memory, n_pixels x 16 B (F32) or x 4 B (RGBA8), packed as the tiles are.  HRT_ERR_STATE with no
 * samples. */
hrt_status hrt_accum_resolve(hrt_accum* a, int32_t format, void* d_out, void* stream);
/* The same into caller-owned host memory; synchronous. */
hrt_status hrt_accum_resolve_host(hrt_accum* a, int32_t format, void* out);
/* dst += src (same device, same tile set, same frame identity, disjoint sample ranges). */
hrt_status hrt_accum_merge(hrt_accum* dst, const hrt_accum* src, void* stream);
/* Checkpoint / transport: the raw sums (n_pixels x 4 f32, w = 0) and the sample ranges as [begin, end) pairs of
 * u32 (an end of 2^32 is stored as 0).  *n_ranges = the number of ranges; sums and ranges are written only when
 * cap >= that number (sums may be NULL to ask for the count).  Upload puts them into the accumulator under the
 * identity of (cam, p), whose samples and sample_offset are ignored: an accumulator without samples takes the
 * sums as they are (so download + upload reproduces an accumulator bit for bit), one with samples adds them as
 * a merge does. */
hrt_status hrt_accum_download(hrt_accum* a, float* sums, uint32_t* ranges, uint32_t cap, uint32_t* n_ranges);
hrt_status hrt_accum_upload(hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, const float* sums,
                            const uint32_t* ranges, uint32_t n_ranges);

/* ---- noise estimate and passes over a subset of the tiles ----
 * A HRT_ACCUM_NOISE accumulator keeps, beside the sums, the moment m2 of every pixel; hrt_accum_noise turns it into
 * the relative standard error of each pixel's mean and a mean / max of that per tile, and hrt_accum_add_tiles sends
 * a further pass to chosen tiles alone.  The library holds the mechanism only: which tiles get another pass is the
 * caller's policy (examples/render_adaptive.c, Python Accumulator.refine).
 *
 * THE BIT CONTRACT of the noise plane and the error (csrc/accum.h, -ffp-contract=off, all in f32):
 *   - a sum's value is luma(s) = (s.x + s.y) + s.z; Y_c is a chunk sum's value and n_c the chunk's sample count in
 *     the pass's schedule (hrt_debug_sample_chunks);
 *   - a pass's moment is the terms (Y_c * Y_c) * (1.0f / (float)n_c) added in chunk order starting from chunk 0's,
 *     and the plane takes it as ONE addend, m2 = m2 + pass_moment; hrt_accum_merge does dst.m2 + src.m2;
 *   - a tile keeps the sample ranges it holds (N samples) and K, the number of chunks added to it;
 *   - with Y = luma(acc): var = max((m2 - (Y * Y) * (1 / N)) * (1 / (K - 1)), 0) and
 *     err = sqrtf(var * (1 / N)) / max(Y * (1 / N), floor); K < 2 gives +inf.  floor > 0 is the caller's, in units of
 *     the mean of Y: darker pixels are measured against it (a black pixel's error is 0);
 *   - a tile's mean and max: thread j of 256 folds the errors of pixels j, j + 256, ... of the tile's packed order,
 *     in order, from 0; then x[j] = x[j] (op) x[j + s] for s = 128 ... 1; mean = x[0] * (1.0f / (float)pixels).
 *     +inf propagates into both.
 * var is the weighted batch-means estimate of one sample's variance (unbiased for chunks of unequal sizes), so err
 * estimates the relative standard error of the pixel's mean.  In f32 it bottoms out near 2e-4: below
 * that a pixel is converged, not measured.
 * Subset passes: for each selected tile's pixels the pass sum is exactly hrt_render's for those params, followed by
 * acc + pass_sum (and m2 + pass_moment).  A tile's pixels and its noise plane are a function of THAT TILE's pass
 * schedule alone: never of which other tiles took part in a pass, of the tile split or of the device.  Each tile
 * resolves with its own sample count.
 * While the tiles hold different passes: hrt_accum_samples is HRT_ERR_STATE (hrt_accum_tile_samples answers);
 * hrt_accum_add is allowed and its range is checked against every tile; hrt_accum_add_resolve, merge, download and
 * upload are HRT_ERR_UNSUPPORTED; a resolve needs samples in every tile (HRT_ERR_STATE).  Once every tile holds the
 * same ranges and chunk count again, the accumulator is an ordinary one again.
 * HRT_ACCUM_NOISE accumulators otherwise behave as plain ones (same sums, same frames, bit for bit) except: merge
 * needs both sides to have the flag (HRT_ERR_INVALID_ARG otherwise) and also adds m2 and K; hrt_accum_download works,
 * but the noise plane and K do not travel, so hrt_accum_upload into one is HRT_ERR_UNSUPPORTED.  These calls keep
 * their refusals: the whole state (noise plane, K, per-tile ranges, feature planes) travels through hrt_accum_snapshot /
 * hrt_accum_restore, and tiles that hold different passes merge through hrt_accum_merge_tiles.  hrt_accum_reset also clears
 * m2, K and the per-tile ranges.  Frame identity, streams and the watchdog's invalid state apply unchanged. */
/* Render samples [p->sample_offset, + p->samples) of tiles[idx[0..n)] of the accumulator only (indices into the
 * tile list it was created with) and add them: one megakernel launch and one accumulate kernel, whatever n.
 * HRT_ERR_INVALID_ARG, with nothing changed: n == 0, an index out of range or given twice, a range that overlaps
 * the ranges of ANY selected tile. */
hrt_status hrt_accum_add_tiles(hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, const uint32_t* idx, uint32_t n,
                               void* stream, hrt_render_stats* stats);
/* One tile's record of hrt_accum_noise (a struct the CALLER allocates an array of; 24 bytes). */
typedef struct hrt_tile_noise hrt_tile_noise;
struct hrt_tile_noise {
  float mean, max;  /* of the tile's per-pixel err */
  uint64_t samples; /* N of the tile */
  uint64_t chunks;  /* K of the tile */
};
/* The error of every pixel to d_err (device memory, n_pixels floats packed as the tiles are; may be NULL) and one
 * record per tile to tiles_out (host memory, n_tiles records); synchronises `stream`.  floor <= 0 or NaN is
 * HRT_ERR_INVALID_ARG; an accumulator without HRT_ACCUM_NOISE, or without samples, HRT_ERR_STATE.  A tile without
 * samples (or with one chunk) reports +inf. */
hrt_status hrt_accum_noise(hrt_accum* a, float floor, float* d_err, void* stream, hrt_tile_noise* tiles_out);
/* The samples each tile holds (n_tiles values). */
hrt_status hrt_accum_tile_samples(const hrt_accum* a, uint64_t* per_tile);

/* ---- variance-guided preview filter ----
 * An opt-in resolve of a HRT_ACCUM_NOISE accumulator for previews of noisy scenes: an edge-stopping a-trous filter
 * whose tolerance at each pixel comes from the noise plane.  It uses no feature buffers (albedo, normal, depth), so it
 * blurs detail that is smaller than its footprint and no noisier than its surroundings: it is never a default
 * (README.md, DESIGN.md section 6.7 say where it helps and where it hurts).
 *
 * THE BIT CONTRACT of the filtered frame (csrc/filter.h, -ffp-contract=off, IEEE '/' and sqrtf, all in f32):
 *   Domain: the pixels the accumulator's tiles cover.  A neighbour that is off the image, or covered by no tile, is
 *   ABSENT and contributes to no sum.  An accumulator whose tiles overlap is HRT_ERR_UNSUPPORTED.
 *   Inputs of pixel p, with inv_n = 1.0f / (float)N and inv_k1 = 1.0f / (float)(K - 1) of p's tile:
 *     c_p = (acc.x * inv_n, acc.y * inv_n, acc.z * inv_n), the linear radiance; l_p = (c_p.x + c_p.y) + c_p.z;
 *     v_p = var * inv_n with var of the noise contract above (Y = luma(acc_p)): the variance of the mean.
 *   Iterations i = 0 .. iterations - 1 with step s = 1 << i; each reads the planes (c, v) of the previous one and is
 *   never in place:
 *     1. Prefiltered variance: num = den = 0.0f; for dy = -1..1 (outer), dx = -1..1 (inner) over present
 *        q = p + (dx, dy): g = G[dy + 1] * G[dx + 1] with G = {1, 2, 1}; num = num + g * v_q, then den = den + g;
 *        vb = num / den.
 *     2. Scale: r = 1.0f / (sigma * sqrtf(vb) + 1e-6f).
 *     3. Taps: sc = (0, 0, 0), sv = 0, sw = 0; for dy = -2..2 (outer), dx = -2..2 (inner) over present
 *        q = p + s * (dx, dy), the centre included at its place in the order: d = fabsf(l_q - l_p) * r;
 *        t = (1.0f - d * 0.5f) if that is > 0, else 0; e = t * t, then e = e * e; w = (H[dy + 2] * H[dx + 2]) * e with
 *        H = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f}; sc = sc + w * c_q per channel, sv = sv + (w * w) * v_q,
 *        sw = sw + w.
 *     4. Result: c' = sc / sw per channel, v' = sv / (sw * sw); if sw == 0 (only reachable through NaN), c' = c_p and
 *        v' = v_p.
 *   Output: sqrtf(c'.x), sqrtf(c'.y), sqrtf(c'.z), 1 as HRT_ACCUM_F32, or the PPM rule on that as HRT_ACCUM_RGBA8,
 *   packed as the tiles are.
 * So the filtered frame is a function of the sums, the planes and the covered pixel set: it does not depend on how
 * that set is cut into tiles.  A filtered resolve never writes the sums or m2: resolve, noise and later passes give
 * the bits they would have given.  Tiles that hold different passes are supported (each with its own N and K).
 * Two raster planes of 16 B per pixel of the tiles' bounding box are allocated by the first filtered resolve and
 * freed with the accumulator; the work is stream-ordered on `stream`.
 * Errors, each changing nothing: HRT_ERR_INVALID_ARG for iterations outside [1, 5], sigma <= 0 or NaN, an unknown
 * format, null pointers; HRT_ERR_STATE for an accumulator without HRT_ACCUM_NOISE, without samples, with a tile that
 * holds no samples or fewer than 2 chunks, or in the watchdog's invalid state. */
typedef struct hrt_filter_params hrt_filter_params;
struct hrt_filter_params { /* 8 bytes */
  uint32_t iterations; /* 1 .. 5: footprint radius 2 * (2^iterations - 1) px */
  float sigma;         /* > 0: luminance tolerance in standard errors; 4 is a good start */
};
hrt_status hrt_accum_resolve_filtered(hrt_accum* a, const hrt_filter_params* f, int32_t format, void* d_out, void* stream);
/* ... into HOST memory; waits for the device as hrt_accum_resolve_host does */
hrt_status hrt_accum_resolve_filtered_host(hrt_accum* a, const hrt_filter_params* f, int32_t format, void* out);

/* ---- first-hit feature planes ----
 * A HRT_ACCUM_FEATURES accumulator (independent of HRT_ACCUM_NOISE) keeps, beside the sums, two planes of first-hit
 * features, packed as the sums are, zero at creation: inputs for the guided filter below or for an external denoiser.
 * THE BIT CONTRACT of the feature planes (csrc/feature_pass.h, -ffp-contract=off, all in f32):
 *   The features of sample k of a pixel are those of the FIRST hit of the path a radiance sample k of that pixel
 *   traces: the same camera ray (the same draws from (seed, pixel, k)), the closest hit over the reference node stream
 *   from t_min, a ConstantMedium drawing from its own keyed sub-stream as in a render.
 *     hit    = 1.0f on a hit, 0.0f on a miss;
 *     albedo = Lambertian / Isotropic: the texture's value at the hit; Metal: its albedo; Dielectric: (1, 1, 1);
 *              DiffuseLight: the emit texture's value, unclamped; a miss: the params' background;
 *     normal = the hit record's world-space normal, which faces the ray; (0, 0, 0) for a medium hit and a miss;
 *     depth  = t * sqrtf(dot(d, d)) of the camera ray (origin o, direction d) on a hit, 0 on a miss.
 *   One hrt_accum_add_features sums its samples of a pixel in index order into fa = (albedo.xyz, hit) and
 *   fn = (normal.xyz, depth), each from 0.0f, and the planes take the pass sum as ONE addend, plane = plane + pass_sum;
 *   hrt_accum_merge does dst + src.
 * So the planes are a function of the feature pass schedule alone: they never depend on the tile split, the device
 * count or the radiance passes.  A feature pass never touches the sums, m2, K or the radiance ranges, and every other
 * call returns the bits it would have returned.  The accumulator keeps the feature samples it holds as its own sorted,
 * disjoint, coalesced range list (every feature pass covers every tile); the frame identity is shared with the radiance
 * passes, and the first call of either kind fixes it.  Plans that are approximate (HRT_RENDER_FAST_CULL,
 * HRT_RENDER_SAH) are HRT_ERR_UNSUPPORTED.  hrt_accum_reset clears planes and ranges; hrt_accum_merge needs both sides
 * to have the flag (HRT_ERR_INVALID_ARG otherwise) and adds planes and ranges under the same disjointness rule;
 * hrt_accum_download / _upload carry the sums only and leave the feature planes alone. */
/* Samples [p->sample_offset, + p->samples) of every pixel of every tile: one launch.  An overlap with a held feature
 * range, samples == 0 or an end above 2^32: HRT_ERR_INVALID_ARG; no HRT_ACCUM_FEATURES: HRT_ERR_STATE; nothing changes. */
hrt_status hrt_accum_add_features(hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p, void* stream);
hrt_status hrt_accum_feature_samples(const hrt_accum* a, uint64_t* samples);
/* The mean planes of the NF feature samples held, packed, 16 B per pixel each, into DEVICE memory; either pointer may
 * be NULL, not both.  With inv = 1.0f / (float)NF: albedo = (fa.xyz * inv, fa.w * inv) (w: the hit fraction);
 * normal = (fn.xyz * inv, z), z = fa.w > 0 ? fn.w * (1.0f / fa.w) : 0 (the mean depth of the hits).  No feature
 * samples: HRT_ERR_STATE. */
hrt_status hrt_accum_features(hrt_accum* a, void* d_albedo, void* d_normal, void* stream);
/* ... into HOST memory; waits for the device */
hrt_status hrt_accum_features_host(hrt_accum* a, float* albedo, float* normal);

/* ---- feature-guided preview filter ----
 * hrt_accum_resolve_filtered with edge-stopping terms on the mean feature planes, for an accumulator created with
 * HRT_ACCUM_NOISE | HRT_ACCUM_FEATURES that holds at least one feature sample (and meets the filtered resolve's
 * preconditions; HRT_ERR_STATE otherwise).
 * THE BIT CONTRACT of the guided frame (csrc/filter.h): exactly the filtered frame's iteration (the same domain, absent
 * pixels, prefiltered variance, r, tap order, H, sv and sw).  After the luminance term e = (t * t)^2 of a tap q at
 * pixel p the ENABLED terms follow in this order, with k_f = 1.0f / tolerance_f computed once on the host:
 *   normal: d = ((dx * dx + dy * dy) + dz * dz) of n_q - n_p; t = at_least(1.0f - d * k_n, 0); e = e * (t * t);
 *   albedo: the same on a_q - a_p with k_a;
 *   depth:  d = fabsf(z_q - z_p) / ((z_q + z_p) + 1e-6f); t = at_least(1.0f - d * k_z, 0); e = e * (t * t);
 * (a, n, z: the mean planes of hrt_accum_features, constant across iterations).  A tolerance of 0 switches its term
 * off: the term is skipped, not multiplied by one, so with all three 0 the frame equals hrt_accum_resolve_filtered's
 * bit for bit.  A tolerance above 0 is the feature distance at which the term's weight reaches 0; negative or NaN is
 * HRT_ERR_INVALID_ARG.  The frame is a function of the sums, m2, (N, K) per tile, the feature planes and the covered
 * pixel set: it does not depend on the tile cut, and the resolve writes none of them.  Two further rasters of 16 B per
 * pixel of the tiles' bounding box are allocated by the first guided resolve and freed with the accumulator. */
typedef struct hrt_guided_params hrt_guided_params;
struct hrt_guided_params { /* 20 bytes */
  uint32_t iterations;         /* as hrt_filter_params */
  float sigma;                 /* as hrt_filter_params */
  float normal, albedo, depth; /* tolerances; 0: the term is off */
};
hrt_status hrt_accum_resolve_guided(hrt_accum* a, const hrt_guided_params* g, int32_t format, void* d_out, void* stream);
/* ... into HOST memory; waits for the device as hrt_accum_resolve_host does */
hrt_status hrt_accum_resolve_guided_host(hrt_accum* a, const hrt_guided_params* g, int32_t format, void* out);

/* ---- guided resolve with options: demodulation by the first-hit albedo ----
 * hrt_accum_resolve_guided with a flags word.  With flags == 0 the frame, the preconditions and every status are
 * hrt_accum_resolve_guided's, bit for bit (and with all three tolerances 0 as well, hrt_accum_resolve_filtered's).
 * HRT_GUIDED_DEMODULATE: the filter runs on the radiance DIVIDED by the first-hit albedo and the albedo is multiplied
 * back afterwards, so the filter averages irradiance across texture edges and the texture returns at full sharpness.
 * An opt-in, never a default (README.md, DESIGN.md section 6.10 say where it helps and where it does not).
 * THE BIT CONTRACT of the demodulated frame (csrc/filter.h; f32, -ffp-contract=off, IEEE '/'), for a pixel p, with a_p
 * the xyz of the mean albedo plane (exactly the bits hrt_accum_features returns) and floor = albedo_floor:
 *   1. Divisor: m_p = (at_least(a_p.x, floor), at_least(a_p.y, floor), at_least(a_p.z, floor)), at_least(x, lo) being
 *      x > lo ? x : lo, so a NaN albedo gives floor.
 *   2. Demodulated input, in place of the guided frame's (c_p, v_p): d_p = (c_p.x / m_p.x, c_p.y / m_p.y, c_p.z / m_p.z);
 *      l = (c_p.x + c_p.y) + c_p.z and l' the same of d_p; g = l > 0 ? l' / l : 0.0f; v'_p = v_p * (g * g).  This keeps
 *      the relative standard error of the luminance and is exact for a grey albedo.
 *   3. Iterations: exactly the guided frame's on the planes (d, v'): the same order, prefilter, r, taps, H, sv and sw;
 *      the enabled feature terms are unchanged and read the same mean planes.
 *   4. Output: c'' = (d'.x * m_p.x, d'.y * m_p.y, d'.z * m_p.z) of the last iteration's d', then sqrtf per channel and
 *      alpha 1, or the PPM rule on that.  The sw == 0 escape returns the demodulated input pixel, which is remodulated
 *      like any other.
 * The demodulated frame is a function of the sums, m2, (N, K) per tile, the feature planes, the floor and the covered
 * pixel set: it does not depend on the tile cut, and the resolve writes none of its inputs.  With the flag set and all
 * three tolerances 0 the frame is the demodulated variance-only filter, a legal setting.  The option is a parameter of
 * a resolve, not state: a snapshot does not carry it.  No pass over the frame and no raster is added to the guided
 * resolve's.
 * Errors, each changing nothing: hrt_accum_resolve_guided's, and HRT_ERR_INVALID_ARG for unknown flag bits, for
 * reserved != 0, and for an albedo_floor that is <= 0 or NaN while HRT_GUIDED_DEMODULATE is set (the floor is not
 * read when it is clear). */
enum { HRT_GUIDED_DEMODULATE = 1 };
typedef struct hrt_guided_ex_params hrt_guided_ex_params;
struct hrt_guided_ex_params { /* 32 bytes */
  uint32_t iterations;         /* as hrt_guided_params */
  float sigma;                 /* as hrt_guided_params */
  float normal, albedo, depth; /* as hrt_guided_params */
  uint32_t flags;              /* HRT_GUIDED_* bits; others: HRT_ERR_INVALID_ARG */
  float albedo_floor;          /* HRT_GUIDED_DEMODULATE: > 0; 0.01 is a good start */
  uint32_t reserved;           /* 0 */
};
hrt_status hrt_accum_resolve_guided_ex(hrt_accum* a, const hrt_guided_ex_params* g, int32_t format, void* d_out, void* stream);
/* ... into HOST memory; waits for the device as hrt_accum_resolve_host does */
hrt_status hrt_accum_resolve_guided_ex_host(hrt_accum* a, const hrt_guided_ex_params* g, int32_t format, void* out);

/* ---- noise estimate of the FILTERED frame ----
 * hrt_accum_noise for the frame a filtered resolve shows: every a-trous iteration carries the variance of the filtered
 * mean, v' = sv / (sw * sw), and this call turns the last iteration's into a per-pixel relative standard error and
 * per-tile records, so that a caller who looks at the filtered preview can stop refining on ITS error (Python
 * Accumulator.refine_filtered, examples/render_adaptive_filtered.c).  g is exactly hrt_accum_resolve_guided_ex's
 * parameter block and names the resolve whose frame is estimated; all tolerances 0 and flags 0 is
 * hrt_accum_resolve_filtered's frame.  No frame is written and no pass is added: the iterations are the resolve's own,
 * the last one writing the error where the frame's pixel would have gone, then one reduce the size of hrt_accum_noise's.
 * THE BIT CONTRACT (csrc/filter.h; f32, -ffp-contract=off, IEEE '/' and sqrtf).  Let (c', v') be pixel p's output of the
 * LAST iteration of the resolve g describes; the iterations are those of the contracts above, unchanged:
 *   - flags == 0: l' = (c'.x + c'.y) + c'.z; err = sqrtf(v') / at_least(l', floor);
 *   - HRT_GUIDED_DEMODULATE: the last iteration yields d' and v' in demodulated units and c'' = (d'.x * m_p.x, d'.y *
 *     m_p.y, d'.z * m_p.z) (step 4 above); l_d = (d'.x + d'.y) + d'.z and l'' the same of c''; gr = l_d > 0 ? l'' / l_d
 *     : 0.0f; v'' = v' * (gr * gr); err = sqrtf(v'') / at_least(l'', floor): the mirror of step 2 above;
 *   - the sw == 0 escape yields the input pixel's (c, v) and goes through the same expression;
 *   - a tile's mean and max are exactly hrt_accum_noise's reduction over the tile's packed errs: thread j of 256 folds
 *     pixels j, j + 256, ... in order from 0, then x[j] = x[j] (op) x[j + s] for s = 128 ... 1, mean = x[0] * (1.0f /
 *     (float)pixels); NaN and +inf propagate as they do there.
 * The per-pixel err is a function of the sums, m2, (N, K) per tile, the feature planes, g, floor and the covered pixel
 * set: it does not depend on the tile cut.  UNLIKE hrt_accum_noise, a tile's record DOES depend on its neighbours'
 * passes, because the filter's footprint crosses tile edges.  The call writes none of its inputs (the rasters and the
 * error plane it uses are scratch, not part of a snapshot): every later call returns the bits and the status it would
 * have returned without it.
 * WHAT IT IS AND IS NOT: v' propagates the input variances through the tap weights as if the taps were independent and
 * the weights fixed.  It estimates the VARIANCE of the filtered frame, not its bias (blur): texture or geometry smaller
 * than the footprint is averaged away and this estimate does not see it.  So err is a lower bound on the shown frame's
 * error, tightest where the filter's assumptions hold (README.md and DESIGN.md section 6.11 give the calibration).  An
 * opt-in policy input, never a default.
 * d_err: device memory, n_pixels floats packed as the tiles are, or NULL (the accumulator then keeps the plane itself,
 * 4 B per pixel, made by the first such call and freed with it).  tiles_out: host memory, n_tiles records; samples and
 * chunks are the tile's N and K, as in hrt_accum_noise.  Synchronises `stream`, as hrt_accum_noise does.
 * Errors, each changing nothing: every precondition and status of hrt_accum_resolve_guided_ex, except that the feature
 * planes (HRT_ACCUM_FEATURES) and feature samples are required only when a tolerance is > 0 or the flag is set:
 * hrt_accum_resolve_guided_ex refuses an accumulator without HRT_ACCUM_FEATURES even at all-zero tolerances, while this
 * call takes the all-off case through the variance-only filter (the same bits), whose preconditions are
 * hrt_accum_resolve_filtered's, so a HRT_ACCUM_NOISE-only accumulator is accepted.  In particular a tile with fewer than
 * 2 chunks is HRT_ERR_STATE (hrt_accum_noise answers +inf for it).  HRT_ERR_INVALID_ARG for floor <= 0 or NaN and for a
 * null g or tiles_out. */
hrt_status hrt_accum_noise_filtered(hrt_accum* a, const hrt_guided_ex_params* g, float floor, float* d_err, void* stream,
                                    hrt_tile_noise* tiles_out);

/* ---- snapshots: checkpoint, restore and transport of the WHOLE accumulator state ----
 * hrt_accum_snapshot writes everything the accumulator's later answers depend on into one self-describing blob in host
 * memory; hrt_accum_restore puts it into an empty accumulator created with the same width, height, tile list and flags
 * (on the same committed scene, as hrt_accum_upload requires; the blob carries no scene fingerprint).
 * THE RESTORE CONTRACT: after a restore every later call returns the bits, and the status, it would have returned on the
 * snapshotted accumulator: resolve, resolve_filtered, resolve_guided, resolve_guided_ex, noise, tile_samples, samples, feature_samples,
 * features, and every later add, add_tiles, add_features and merge* with its acceptance or refusal.  So "render S1,
 * snapshot, destroy, create, restore, render S2" equals "render S1, render S2" bit for bit in every plane.  The filters'
 * raster buffers are scratch and are not part of a snapshot.
 *
 * THE LAYOUT (format version 1; every integer little-endian, u32 unless said; csrc/accum_snapshot.h is the codec):
 *     0  magic 0x53545248 ("HRTS"), version 1
 *     8  u64 bytes: the size of the whole blob, checksum included
 *    16  flags (HRT_ACCUM_NOISE | HRT_ACCUM_FEATURES), width, height, n_tiles
 *    32  u64 n_pixels: the sum of w * h over the tiles
 *    40  has_identity (0 / 1), n_records (1, or n_tiles while the tiles hold different passes), n_feature_ranges, 0
 *    56  the frame identity, 128 bytes (all 0 when has_identity is 0): hrt_camera's 96 bytes, max_depth, flags,
 *        f32 t_min, f32 background[3], u64 seed
 *   184  the tile list: n_tiles x (x, y, w, h)
 *        the radiance ledger: n_records x { u64 K (chunks), u64 n_ranges, n_ranges x (u64 begin, u64 end) }, each list
 *        sorted, disjoint, coalesced, non-empty ranges with end <= 2^32 (u64: 2^32 needs no wrap rule); a record without
 *        ranges has K = 0
 *        the feature ledger: n_feature_ranges x (u64 begin, u64 end), the same rules (0 without HRT_ACCUM_FEATURES)
 *        zeros up to the next multiple of 16
 *        the sums, n_pixels x 16 B, packed as the tiles are
 *        with HRT_ACCUM_NOISE: m2, n_pixels x 4 B, then zeros up to the next multiple of 16
 *        with HRT_ACCUM_FEATURES: fa, then fn, n_pixels x 16 B each
 *        u64 checksum of the W = (bytes - 8) / 8 little-endian u64 words w_0 .. w_{W-1} before it: with
 *        P = 0x100000001B3, four lanes h_i = 0xCBF29CE484222325 + i; word j does h_{j mod 4} = (h_{j mod 4} ^ w_j) * P;
 *        then r = h_0, r = (r * P) ^ h_i for i = 1, 2, 3, r = (r ^ W) * P, checksum = r ^ (r >> 32), all mod 2^64.
 * A blob is untrusted input: the decoder checks every length against `size` before it reads.  MALFORMED, each
 * HRT_ERR_INVALID_ARG: shorter than its header, tile list or ledgers say; wrong magic or version; `size` not the bytes
 * field, or not what the layout adds up to; unknown flags, a width or height outside [2, 65535], no tiles, a tile outside
 * the image, n_pixels not the tiles' sum; ranges unsorted, overlapping, adjacent, empty or past 2^32; n_records neither 1
 * nor n_tiles; K without ranges; feature ranges without the flag; has_identity == 0 together with samples or identity
 * bytes; a bad checksum.
 * Errors, each changing nothing: a snapshot of an accumulator in the watchdog's invalid state is HRT_ERR_STATE; a restore
 * into an accumulator that holds radiance or feature samples (reset it first), or that is invalid, is HRT_ERR_STATE; a
 * malformed blob, or one whose flags, width, height or tile list are not the accumulator's, is HRT_ERR_INVALID_ARG.
 * hrt_accum_snapshot waits for the device, as hrt_accum_download does; hrt_accum_restore is synchronous. */
/* *size = the snapshot's bytes.  out == NULL: only that.  Otherwise cap >= *size, else HRT_ERR_INVALID_ARG with nothing
 * written to out. */
hrt_status hrt_accum_snapshot(hrt_accum* a, void* out, uint64_t cap, uint64_t* size);
hrt_status hrt_accum_restore(hrt_accum* a, const void* blob, uint64_t size);
/* What an accumulator must be created with to take this blob (a struct the CALLER allocates; 40 bytes). */
typedef struct hrt_snapshot_info hrt_snapshot_info;
struct hrt_snapshot_info {
  uint32_t version, flags, width, height, n_tiles;
  uint32_t uniform; /* 1: every tile holds the same passes (n_records == 1) */
  uint64_t n_pixels, bytes;
};
/* Validates the blob as a restore does (no device involved) and describes it; the tile list goes to `tiles` when
 * cap >= n_tiles (tiles may be NULL with cap 0 to ask for n_tiles first). */
hrt_status hrt_accum_snapshot_info(const void* blob, uint64_t size, hrt_snapshot_info* info, hrt_tile* tiles, uint32_t cap);

/* ---- merging accumulators whose tiles hold different passes ----
 * hrt_accum_merge for accumulators whose tiles may hold different passes, on either side, with or without the noise and
 * feature planes.  Preconditions as hrt_accum_merge's: the same device, image size and tile list, HRT_ACCUM_NOISE and
 * HRT_ACCUM_FEATURES equal on both sides, the same frame identity, both usable.
 * THE CONTRACT:
 *   - for every tile t, src's ranges of t must be disjoint from dst's ranges of t: otherwise HRT_ERR_INVALID_ARG and
 *     nothing changes;
 *   - a tile for which src holds no samples is NOT TOUCHED: its sums, its m2, its ranges and its K are never written (a
 *     -0.0f or NaN bit pattern survives);
 *   - every other tile takes acc = acc + src.acc per channel (dst's operand first) and m2 = m2 + src.m2, its ranges
 *     become the union and K = K + K_src;
 *   - the feature planes and the feature ranges merge exactly as in hrt_accum_merge (every tile, dst + src);
 *   - if every tile then holds the same ranges and K, the accumulator is an ordinary one again (hrt_accum_samples,
 *     download, merge work);
 *   - two accumulators whose tiles each hold the same passes give hrt_accum_merge's bits.
 * One kernel launch for sums and m2 whatever the subset, stream-ordered on `stream`; the host bookkeeping is updated at
 * call time. */
hrt_status hrt_accum_merge_tiles(hrt_accum* dst, const hrt_accum* src, void* stream);

/* ---- ray queries: the closest hits of caller-supplied rays ----
 * Everything above starts at a pixel.  hrt_scene_intersect answers "what does this ray hit?" for rays the caller
 * keeps in device memory: picking, autofocus (examples/render_autofocus.c), visibility between two points, baking, a
 * depth map from another camera model, the segments of a path replayed.  hrt_camera_rays writes the camera rays a
 * render's samples start with, so the two together are a frame's first hits.
 *
 * THE BIT CONTRACT of a hit (csrc/query.h, -ffp-contract=off, all in f32):
 *   Closest hit.  Ray i's answer is the closest hit of world.hit(ray, t_min, t_max) as a render's segment with that
 *   origin, direction and time computes it: the walk the feature pass makes (lane.h trace over the reference node
 *   stream from t_min, the closest starting at t_max), then the hit record (lane.h make_record; hit_record.rs).  The
 *   interval is the reference's at both ends: a root t is refused when t < t_min or t_max < t (sphere.rs:53-55,
 *   moving_sphere.rs:74-76, rect.rs:61), so t == t_min and t == t_max are both accepted by the primitive, and a later
 *   primitive replaces an earlier one at an equal t.  The reference asks a primitive only after its boxes
 *   (bvh_node.rs:104-106), and aabb.rs refuses a box when `t_max <= t_min` holds of its clipped interval: a rect lies in
 *   the face of its own box (the 0.0002-thick slab of rect.rs:97-107, a Cuboid's box), whose entry time (bound - o) * (1 / d)
 *   can round onto the rect's t = (k - o) / d or past it, so a rect's hit at exactly t_max or t_min can be the
 *   reference's miss, and is then a miss here (measured: 0 to 4% of such rays on scenes with rects, none on spheres;
 *   DESIGN.md "Queries against the oracle").  The direction is used as given (t is in units of its length).
 *   Culling.  Boxes are culled by the scene's exact mode (the reference's box test plus culling that provably drops
 *   no accepted hit) when [time0, time1] of the params lies inside the interval the scene's BVH boxes were built for,
 *   and by the reference's test alone otherwise or under HRT_QUERY_REFERENCE_CULL.  Both give the same hits; there is
 *   no approximate mode for queries.
 *   The record.  t, point, normal, u, v and the front-face bit are the hit record's; the normal faces the ray.  u and
 *   v are ALWAYS computed (a render computes a sphere's only under an image texture).
 *   Ids.  prim is the primitive's index in reference pre-order (hrt_debug_prim_record order 0), for sphere scenes and
 *   general scenes alike: the pre-order of world.hit's recursion (left before right, a Cuboid's six sides in their list
 *   order, through instances) over the primitives OUTSIDE every medium boundary; the boundaries' own primitives are
 *   numbered after all of those and no record names one.  material is the material's id: a constructor's id, or for a
 *   medium's phase function the number of constructed materials plus the medium's index.  A scatter inside a
 *   ConstantMedium sets HRT_HIT_MEDIUM: prim is then the medium's index, which counts the ConstantMedium nodes in that
 *   same pre-order (NOT in creation order, which is the medium id that keys the draws below), normal (0, 0, 0),
 *   u = v = 0 and front clear, as a render's record has it.
 *   Medium draws.  A ConstantMedium draws its scatter distance from the sub-stream keyed by (params.seed, ray.pixel,
 *   ray.sample, ray.segment, medium id), exactly a render's key for segment number `segment` of sample `sample` (the
 *   ABSOLUTE sample index) of pixel `pixel` (y * width + x): a query with a path's key repeats that segment's draw.
 *   HRT_QUERY_SKIP_MEDIA makes every medium transparent.
 *   Miss.  flags = 0, t = the ray's t_max, prim = material = 0xFFFFFFFF, every other field +0.
 *   Non-finite records.  A valid ray can still take the reference's arithmetic to a NaN: a ray in a rect's plane
 *   (t = 0 / 0), a direction of length 1e18 (sphere.rs's half_b^2 - a c = inf - inf), an origin so far away that
 *   (at(root) - center) / radius leaves [-1, 1] and sphere.rs's acos gives a NaN v.  Such a record is the reference's,
 *   field by field: a field that is NaN there is a NaN here, of unspecified sign and payload; every other field is equal.
 *   Invalid ray.  A ray with a non-finite value in origin, direction, time or t_min, with a NaN t_max, with the
 *   direction (0, 0, 0), for which t_min < t_max does not hold, or whose time lies outside [time0, time1], is not
 *   traced: flags = HRT_HIT_INVALID, prim = material = 0xFFFFFFFF, every other field +0.
 *   What a result depends on.  Hit i is a function of ray i, the params and the committed scene ALONE: never of n, of
 *   the ray's position in the batch, of the other rays, of HRT_QUERY_NO_LDS or of the device.  d_hits[n ..] is never
 *   written.  The call writes nothing in the scene and is re-entrant as the renders are; the work is asynchronous on
 *   `stream`.
 * d_rays and d_hits are device memory, n records of 48 bytes each, 16-byte aligned, and must not overlap.
 * Errors, each changing nothing and answered before any device call: HRT_ERR_INVALID_ARG for a null scene, params or
 * buffer (n == 0 is HRT_OK whatever the buffers, and launches nothing), a misaligned buffer, unknown flags,
 * reserved != 0, time0 <= time1 not holding or a non-finite bound, n >= 2^32; HRT_ERR_STATE for an uncommitted scene. */
typedef struct hrt_ray hrt_ray;
struct hrt_ray { /* 48 bytes */
  float origin[3];
  float t_min;
  float direction[3]; /* need not be normalised */
  float t_max;        /* +inf allowed */
  float time;
  uint32_t pixel, sample, segment; /* the key of a ConstantMedium's draw (above); 0, 0, 0 is fine */
};
typedef struct hrt_hit hrt_hit;
struct hrt_hit { /* 48 bytes: the reference's HitRecord (hit_record.rs) and the ids */
  float t;
  uint32_t prim;
  uint32_t material;
  uint32_t flags; /* HRT_HIT_* */
  float point[3];
  float u;
  float normal[3];
  float v;
};
enum { HRT_HIT_HIT = 1, HRT_HIT_FRONT = 2, HRT_HIT_MEDIUM = 4, HRT_HIT_INVALID = 8 };
enum {
  HRT_QUERY_SKIP_MEDIA = 1,    /* ConstantMedium nodes are transparent */
  HRT_QUERY_NO_LDS = 2,        /* keep the scene in global memory even when it fits in LDS (A/B; the same hits) */
  HRT_QUERY_REFERENCE_CULL = 4 /* aabb.rs's box test alone (the same hits) */
};
typedef struct hrt_query_params hrt_query_params;
struct hrt_query_params { /* 24 bytes */
  uint32_t flags;    /* HRT_QUERY_* bits */
  uint32_t reserved; /* 0 */
  float time0, time1; /* the interval the rays' times lie in: time0 <= time1, both finite */
  uint64_t seed;      /* with (pixel, sample, segment) of a ray: the key of a medium's draw */
};
hrt_status hrt_scene_intersect(hrt_scene* s, const hrt_query_params* q, const hrt_ray* d_rays, uint64_t n, hrt_hit* d_hits,
                               void* stream);
/* ... with rays and hits in HOST memory: copies in, runs the device path on the scene's device, copies out; synchronous */
hrt_status hrt_scene_intersect_host(hrt_scene* s, const hrt_query_params* q, const hrt_ray* rays, uint64_t n, hrt_hit* hits);
/* The camera rays a render starts with: for every pixel of `tiles` (packed as hrt_render_tiles_device packs them) and
 * k in [0, p->samples), ray (packed pixel index) * p->samples + k is the ray a radiance sample p->sample_offset + k of
 * that pixel draws (lane.h start_sample: jitter, lens point, shutter time, from (p->seed, pixel, sample)), with
 * t_min = p->t_min, t_max = +inf and key (y * width + x, p->sample_offset + k, 0).  So hrt_camera_rays followed by
 * hrt_scene_intersect with p->seed and the camera's shutter as [time0, time1] gives the feature pass's first hits,
 * sample by sample: hit, normal, and depth = t * sqrtf(dot(d, d)).  d_rays: device memory, (the tiles' pixels) x
 * p->samples records, 16-byte aligned.  The checks are the render calls' (width, height, samples, known flags, the
 * shutter, tiles inside the image); p->flags select nothing here.  More than 2^32 - 1 rays: HRT_ERR_INVALID_ARG.  A
 * call with more than one tile reads its tile table from host memory and waits for `stream` before it returns. */
hrt_status hrt_camera_rays(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p, const hrt_tile* tiles,
                           uint32_t n_tiles, hrt_ray* d_rays, void* stream);
/* ... into HOST memory; synchronous */
hrt_status hrt_camera_rays_host(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p, const hrt_tile* tiles,
                                uint32_t n_tiles, hrt_ray* rays);

/* ---- scatter queries: caller-held paths stepped through the scene's materials ----
 * hrt_scene_intersect is the world.hit of one ray_color step; hrt_scene_scatter is the rest of that step (lane.h shade:
 * background on a miss, else emission, the material's scatter and its texture), for paths the caller keeps in device
 * memory between the calls; hrt_camera_paths starts paths exactly as a render starts its samples.  A custom integrator,
 * per-bounce AOVs, light-path statistics (examples/render_integrator.c; hrt.trace_paths in the Python binding).
 *
 * A PATH is the 48-byte record below: the xoshiro128** state of its random stream, its throughput, its radiance so far,
 * the segments it may still trace and HRT_PATH_* flags.  Path i belongs to ray i and hit i of the same batch.
 *
 * hrt_scene_scatter, for path i, in this order (csrc/scatter.h scatter_step, -ffp-contract=off, all in f32):
 *   1. DONE on entry: nothing of ray i or path i is written.
 *   2. An invalid hit - HRT_HIT_INVALID set, flag bits outside the four HRT_HIT_* ones, HRT_HIT_HIT with a material
 *      that is not below the scene's material count, or other bits without HRT_HIT_HIT (no record hrt_scene_intersect
 *      writes): path flags |= INVALID | DONE and nothing else of the path changes.
 *      The material id is the one field of a caller's record that indexes a table; it is checked before any read.
 *      Everything else in a hit is used as a number.  A path whose four rng words are all 0 is refused the same way:
 *      that is no xoshiro state (it never leaves 0, and the rejection loops of the draws would never end), and
 *      hrt_camera_paths never writes it.  A path that is not DONE with depth_left == 0 (none this library writes) takes
 *      the render's depth cap: flags |= DEPTH | DONE, nothing else changes.
 *   3. A miss (flags 0): radiance = radiance + throughput * background (componentwise; shade()'s expression and order),
 *      flags |= MISSED | DONE.
 *   4. A hit: the record is the step's HitRecord - point, normal, front bit, u, v and material as given, the incoming
 *      direction ray.direction.  The step is lane.h scatter<true> with the scene's material and its texture: it draws
 *      from rng exactly as a render does (random_in_unit_sphere for a Lambertian, a Metal and an Isotropic, one f32 for
 *      a Dielectric, nothing for a DiffuseLight).  radiance += throughput * emitted.  Not scattered (a light, or a
 *      metal ray below the surface): flags |= ABSORBED | DONE.  Scattered: throughput *= attenuation, depth_left -= 1,
 *      ray origin = the hit's point, direction = the scattered direction, segment += 1, t_max = +inf; t_min, time,
 *      pixel and sample are kept; if depth_left is now 0, flags |= DEPTH | DONE (the render's next segment would
 *      return black without a world.hit).
 *   5. A path that becomes DONE in this call has its ray written with t_max = t_min, which hrt_scene_intersect answers
 *      as an invalid ray without a walk: a caller may keep calling both functions on the whole batch, uncompacted.
 *   What a result depends on.  Ray i and path i after the call are a function of ray i, hit i and path i before it,
 *   the params and the committed scene ALONE: never of n, of the position in the batch, of the other records, of where
 *   the kernel keeps the scene's Perlin tables (HRT_SCATTER_PERLIN_LDS=0, an A/B knob) or of the device.  Records [n ..)
 *   are never written.
 *
 * THE BIT CONTRACT with the render.  For a committed scene, a camera and render params p whose flags select no
 * approximate culling: hrt_camera_paths once, then hrt_scene_intersect (seed = p->seed, [time0, time1] = the camera's
 * shutter) and hrt_scene_scatter (background = p->background) in turn until every path is DONE, which takes at most
 * p->max_depth rounds.  Then path (pixel, k)'s radiance is, bit for bit, the radiance a render gives sample
 * p->sample_offset + k of that pixel; sqrtf(radiance * 1.0f) is hrt_render's pixel for samples = 1 and that sample
 * offset; and the number of valid, not-DONE rays handed to hrt_scene_intersect over all rounds is the render's ray
 * count (hrt_render_stats.segments).  Excluded: a path that meets a non-finite hit (a rect's t = NaN).  The render
 * walks on from a NaN point up to the depth cap; here the next hrt_scene_intersect refuses the ray and the path ends
 * INVALID.  Sphere scenes cannot produce such a hit.
 *
 * d_rays, d_hits and d_paths are device memory, n records of 48 bytes each, 16-byte aligned, none overlapping; rays and
 * paths are read and written in place, hits are read only.  The work is asynchronous on `stream`.
 * Errors, each changing nothing and answered before any device call: HRT_ERR_INVALID_ARG for a null scene, params or
 * buffer (n == 0 is HRT_OK whatever the buffers, and launches nothing), a misaligned buffer, unknown flags, a non-zero
 * reserved word, a non-finite background component, n >= 2^32; HRT_ERR_STATE for an uncommitted scene. */
typedef struct hrt_path hrt_path;
struct hrt_path { /* 48 bytes */
  uint32_t rng[4];     /* the path's xoshiro128** state (hd_math.h Rng s0 .. s3) */
  float throughput[3]; /* the product of the attenuations so far */
  uint32_t depth_left; /* segments the path may still trace */
  float radiance[3];   /* emitted and background light gathered so far */
  uint32_t flags;      /* HRT_PATH_* */
};
enum { HRT_PATH_DONE = 1, HRT_PATH_MISSED = 2, HRT_PATH_ABSORBED = 4, HRT_PATH_DEPTH = 8, HRT_PATH_INVALID = 16 };
typedef struct hrt_scatter_params hrt_scatter_params;
struct hrt_scatter_params { /* 24 bytes */
  uint32_t flags;      /* 0: no flag is defined yet */
  uint32_t reserved;   /* 0 */
  float background[3]; /* what a miss gathers; finite */
  uint32_t reserved2;  /* 0 */
};
hrt_status hrt_scene_scatter(hrt_scene* s, const hrt_scatter_params* sp, hrt_ray* d_rays, const hrt_hit* d_hits, hrt_path* d_paths,
                             uint64_t n, void* stream);
/* ... with rays, hits and paths in HOST memory: copies in, runs the device path on the scene's device, copies rays and
 * paths out; synchronous */
hrt_status hrt_scene_scatter_host(hrt_scene* s, const hrt_scatter_params* sp, hrt_ray* rays, const hrt_hit* hits, hrt_path* paths,
                                  uint64_t n);
/* hrt_camera_rays' rays, word for word (the same packing, checks and 2^32 limit), and for each ray the path a render's
 * sample starts with (lane.h start_sample): rng after the jitter, lens and shutter draws - which only this call can
 * supply - throughput (1, 1, 1), radiance +0, depth_left = p->max_depth, flags 0.  With p->max_depth == 0 every path
 * starts DONE | DEPTH and its ray carries t_max = t_min (rule 5 above).  d_paths: as d_rays, one path per ray. */
hrt_status hrt_camera_paths(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p, const hrt_tile* tiles,
                            uint32_t n_tiles, hrt_ray* d_rays, hrt_path* d_paths, void* stream);
/* ... into HOST memory; synchronous */
hrt_status hrt_camera_paths_host(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p, const hrt_tile* tiles,
                                 uint32_t n_tiles, hrt_ray* rays, hrt_path* paths);

/* ---- path stepping: intersect and scatter fused, over live lists kept on the device ----
 * hrt_scene_step does for every path of its DOMAIN, in registers, what hrt_scene_intersect followed by hrt_scene_scatter
 * does, `steps` times over, and can write the indices of the paths still live into a device list that the next call takes
 * as its domain: a wavefront loop with no hit records in memory, no pass over finished records and no host round trip
 * (examples/render_wavefront.c; hrt.trace_paths_fused in the Python binding).
 *
 *   1. Domain.  in == NULL: every i in [0, n).  Otherwise the first min(*in->d_count, in->capacity) entries of
 *      in->d_index; the count is read on the device, in stream order.  An entry >= n is skipped and never dereferenced.
 *      Entries must be distinct: with duplicates the records of a duplicated index are unspecified (nothing outside the
 *      arrays is touched).
 *   2. A path DONE on entry: nothing of ray i, path i or hit i is written, and i is not put into `out`.
 *   3. Otherwise, up to `steps` times while the path is not DONE (csrc/step.h step_path): hit = hrt_scene_intersect's
 *      answer for the ray with (seed, time0, time1, flags), the invalid-ray record included; then hrt_scene_scatter's rules
 *      2 to 5 on (ray, hit, path, background), the refusals included (an all-zero rng, depth_left == 0, and an invalid
 *      hit, which ends the path INVALID).  No arithmetic is new: ray i and path i after the call are, bit for bit, those
 *      after `steps` rounds of the two calls.
 *      What a result depends on.  A record after the call is a function of that record before it, the params and the
 *      committed scene ALONE: never of n, of the domain, of the order of the list, of `steps` being split over several
 *      calls, of HRT_STEP_NO_LDS, of where the kernel keeps the Perlin tables (HRT_SCATTER_PERLIN_LDS=0), of the claim
 *      size (HRT_QUERY_CLAIM) or of the device.
 *   4. d_hits, when given: hits[i] is the hit of the LAST intersect the call made for path i (with steps == 1:
 *      hrt_scene_intersect's hit of the ray as it was on entry).  For i outside the domain, or DONE on entry, it is not
 *      written.
 *   5. out, when given: the call sets *out->d_count to 0 in stream order and then appends each i of the domain that was
 *      not DONE on entry and is not DONE after the call, exactly once.  The order is unspecified; the set and the count
 *      are deterministic.  out->capacity >= (in ? in->capacity : n) is checked; out must share neither pointer with in.
 *   6. d_n_rays, when given (8-byte aligned): the call ADDS the number of valid rays it walked, that is rays of live
 *      paths that are no invalid ray.  Summed over a run to completion it is the render's hrt_render_stats.segments.
 *      The caller zeroes it.
 *   7. Records outside the domain, and records [n ..), are never written.
 *   8. The call writes nothing in the scene, is re-entrant as the renders are and asynchronous on `stream`; it allocates
 *      its claim counter in stream order, as hrt_scene_intersect does.
 * d_rays, d_paths and d_hits are device memory, n records of 48 bytes each, 16-byte aligned, none overlapping.  An
 * hrt_path_list is a HOST struct of DEVICE pointers: `capacity` u32 entries at d_index and one u32 at d_count, both 4-byte
 * aligned.
 * Errors, each changing nothing and answered before any device call: HRT_ERR_INVALID_ARG for a null scene, params, rays or
 * paths, a misaligned buffer, unknown flags, steps == 0, reserved != 0, time0 <= time1 not holding or a non-finite bound,
 * a non-finite background component, n >= 2^32, a list with a null pointer, a misaligned pointer or reserved != 0, `out`
 * too small or sharing a pointer with `in`; HRT_ERR_STATE for an uncommitted scene.  n == 0 is HRT_OK whatever the record
 * buffers, launches no kernel and still sets a given *out->d_count to 0. */
enum {
  HRT_STEP_SKIP_MEDIA = 1,    /* the HRT_QUERY_* meanings and values */
  HRT_STEP_NO_LDS = 2,        /* the scene and the Perlin tables stay in global memory (A/B; the same records) */
  HRT_STEP_REFERENCE_CULL = 4
};
typedef struct hrt_step_params hrt_step_params;
struct hrt_step_params { /* 40 bytes */
  uint32_t flags;        /* HRT_STEP_* bits */
  uint32_t steps;        /* >= 1: rounds a live path makes inside the call */
  float time0, time1;    /* as hrt_query_params */
  uint64_t seed;         /* as hrt_query_params */
  float background[3];   /* as hrt_scatter_params; finite */
  uint32_t reserved;     /* 0 */
};
typedef struct hrt_path_list hrt_path_list;
struct hrt_path_list { /* 24 bytes: a HOST struct of DEVICE pointers */
  uint32_t* d_index;   /* capacity entries, 4-byte aligned */
  uint32_t* d_count;   /* one u32 in device memory */
  uint32_t capacity, reserved; /* reserved: 0 */
};
hrt_status hrt_scene_step(hrt_scene* s, const hrt_step_params* sp, hrt_ray* d_rays, hrt_path* d_paths, uint64_t n,
                          hrt_hit* d_hits /* may be NULL */, const hrt_path_list* in /* NULL: every i in [0, n) */,
                          const hrt_path_list* out /* may be NULL */, uint64_t* d_n_rays /* may be NULL */, void* stream);
/* ... with rays, paths, hits and the ray count in HOST memory: the domain is [0, n), there are no lists; copies in, runs
 * the device path on the scene's device, copies rays, paths (and hits) out and ADDS to *n_rays; synchronous */
hrt_status hrt_scene_step_host(hrt_scene* s, const hrt_step_params* sp, hrt_ray* rays, hrt_path* paths, uint64_t n,
                               hrt_hit* hits /* may be NULL */, uint64_t* n_rays /* may be NULL */);

/* ---- caller-traced paths into an accumulator ----
 * hrt_accum_add_paths reduces a finished batch of paths into an accumulator exactly as hrt_accum_add would have added the
 * same samples, so a wavefront loop built on the calls above ends in the accumulator's products: resolve, the noise
 * estimate and refinement, the filters, snapshots and per-tile merges cannot tell the two routes apart.
 *
 *   1. The batch is packed as hrt_camera_paths packs it: with S = p->samples, path (launch pixel i) * S + k is sample
 *      p->sample_offset + k of that pixel, the launch's pixels being those of the accumulator's tiles in order (idx NULL) or
 *      of tiles[idx[0]], tiles[idx[1]], ... .
 *   2. Arithmetic (csrc/accum_paths.h; none of it new).  For each chunk c of the pass's schedule (hrt_debug_sample_chunks)
 *      the chunk sum starts from (0, 0, 0) and adds the radiance of the chunk's paths in sample order, as the render kernels
 *      sum a chunk's samples; the chunk sums then go where a rendered pass's go: the pass sum is the chunk sums added in
 *      chunk order starting from chunk 0's, acc = acc + pass_sum, and with HRT_ACCUM_NOISE m2 = m2 + pass_moment over the
 *      same chunk sums.  A record's radiance is taken as the three floats it holds WHATEVER its flags: an INVALID path's, a
 *      NaN, the radiance of a path the caller stopped early.  What a custom integrator deposits is its own business.
 *   3. Bit contract with hrt_accum_add / hrt_accum_add_tiles.  Take a committed scene, a camera and params whose flags
 *      select no approximate culling; start the paths with hrt_camera_paths on the same tiles in the same order and step
 *      them to completion with hrt_scene_step or the intersect / scatter pair.  This call then leaves the accumulator in
 *      the state the render call with the same arguments leaves it in: sums, noise plane, per-tile sample ranges and chunk
 *      counts K, frame identity; the preview is hrt_accum_add_resolve's.  The scatter contract's exclusion carries over: a
 *      path that met a non-finite hit.
 *   4. Host bookkeeping is hrt_accum_add's own (one function): the identity check and adoption, the range check before
 *      anything is launched, the ledger's record after.
 *   5. What a result depends on.  A pixel after the call is a function of its sums before, its own S records and the
 *      schedule ALONE: never of the tile subset, of the launch shape or of the device.
 *   6. d_live, when given: the call ADDS the number of records that are not HRT_PATH_DONE, which is how a caller learns
 *      without a host round trip that it deposited unfinished paths.  They are deposited all the same.  The caller zeroes it.
 *   7. One kernel launch, asynchronous on `stream`, no intermediate buffer.  A pass over a subset keeps its tile map in the
 *      accumulator, as hrt_accum_merge_tiles keeps its table: one accumulator takes its passes from one thread at a time.
 * Errors, each changing nothing and answered before any device call: HRT_ERR_INVALID_ARG for a null accumulator, camera,
 * params or paths, idx without n_idx or n_idx without idx, n_paths that is not (the tiles' pixels) x p->samples or is
 * >= 2^32, d_paths not 16-byte or d_live not 4-byte aligned, a format outside {-1, HRT_ACCUM_F32, HRT_ACCUM_RGBA8}, a
 * format >= 0 with a null d_out or with idx (a pass over a subset has no preview); hrt_accum_add_tiles' refusals for idx
 * and hrt_accum_add's for the identity, the sample range and the params; HRT_ERR_UNSUPPORTED for a preview when the
 * tiles hold different passes; HRT_ERR_STATE for an accumulator that holds an incomplete pass. */
/* Add the radiance of caller-traced paths as ONE pass: samples [p->sample_offset, + p->samples) of every pixel of the
 * accumulator's tiles (idx NULL) or of tiles[idx[0..n_idx)] alone.  d_paths: the batch hrt_camera_paths(s, cam, p, those
 * tiles in that order) starts, n_paths = (their pixels) x p->samples records, 16-byte aligned, read only. */
hrt_status hrt_accum_add_paths(hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p,
                               const uint32_t* idx /* may be NULL */, uint32_t n_idx,
                               const hrt_path* d_paths, uint64_t n_paths,
                               int32_t format /* -1: no preview */, void* d_out /* may be NULL */,
                               uint32_t* d_live /* may be NULL: ADDS the records that are not PATH_DONE */,
                               void* stream);
/* ... with the paths in HOST memory: copies in, runs the device path, synchronous; *live is added to */
hrt_status hrt_accum_add_paths_host(hrt_accum* a, const hrt_camera* cam, const hrt_render_params* p,
                                    const uint32_t* idx, uint32_t n_idx, const hrt_path* paths, uint64_t n_paths,
                                    uint32_t* live /* may be NULL */);

/* ---- diagnostics ---- */
/* Device occupancy / layout facts of the committed scene (for DESIGN/bench). */
typedef struct hrt_scene_info {
  uint32_t nodes, prims, materials, textures, instances, media;
  uint32_t feature_mask;
  uint32_t blob_bytes;     /* device bytes of the flattened scene */
  uint32_t in_lds;         /* 1 if the megakernel stages the scene in LDS, 2 if only its top levels */
  uint32_t cull_mode;      /* default culling: 2 = exact (reference test + provably safe extra culling) */
  uint32_t sah_stream_len; /* >0: sphere-only scene with the SAH octant streams (8 x this many nodes) */
  /* BvhNode::new sorts of more than 20 objects with equal keys (bvh_node.rs:34): Rust's sort_unstable_by
   * may order such ties differently from this build's stable sort (below 21 objects both are an
   * insertion sort), so 0 means the BVH topology is the reference's for any Rust version */
  uint32_t bvh_tied_sorts;
  uint32_t walk_regrouped; /* sphere scenes: the walk stream's inner boxes are re-grouped (layout.h) */
  uint32_t walk_device_built; /* ... by the device-side build (HRT_WALK_BUILD) */
  uint32_t walk_build_us;  /* the re-grouping's time, host or device (us) */
} hrt_scene_info;
hrt_status hrt_scene_get_info(const hrt_scene* s, hrt_scene_info* info);
/* The last render launch the calling thread made (thread-local, like hrt_last_error): the kernel, its
 * persistent grid and the occupancy answer it was sized by (hipOccupancyMaxActiveBlocksPerMultiprocessor),
 * and the kernel's registers, scratch and LDS (hipFuncGetAttributes), so that a measurement records what
 * ran.  HRT_ERR_STATE before the thread's first launch. */
typedef struct hrt_launch_info {
  char kernel[160];        /* the kernel and its template arguments */
  uint32_t grid, block;    /* workgroups launched, threads per workgroup */
  uint32_t blocks_per_cu;  /* resident workgroups per CU (the occupancy answer) */
  uint32_t cus;            /* compute units of the device */
  uint32_t waves_per_simd; /* blocks_per_cu * block / 64 / 4 */
  uint32_t vgprs;          /* registers per lane */
  uint32_t scratch_bytes;  /* private (scratch) bytes per lane: register spills and stack */
  uint32_t lds_bytes;      /* dynamic LDS per workgroup */
  char knobs[256];         /* the library's A/B environment knobs set in this process ("NAME=value;..."; empty:
                              none).  None of them changes an image's bits (hrt_scene_options does that) */
} hrt_launch_info;
hrt_status hrt_last_launch(hrt_launch_info* out);
/* Write an RGBA f32 frame (w x h, row-major, row 0 = image y 0 = bottom, as the render calls produce;
 * alpha is dropped) to `path` in an HRT_IMAGE_* format. */
hrt_status hrt_image_write(const char* path, const float* rgba, uint32_t w, uint32_t h, int32_t format);
/* Trace ONE path (pixel x,y of the full image; sample index) on the device with the traversal the
 * renderer would use for these params; out[9*i .. 9*i+8] = origin, direction, time, closest t,
 * winner id (bits) of segment i; out[9*max_segments .. +2] = the path's radiance. */
hrt_status hrt_debug_trace_path(hrt_scene* s, const hrt_camera* cam, const hrt_render_params* p, uint32_t x,
                                uint32_t y, uint32_t sample, uint32_t max_segments, float* out,
                                uint32_t* n_segments);
/* The flattened scene as the kernels see it (layout.h sections inside one blob), for host-side
 * inspection and for tests/native/lane_sim.hip, which runs the kernels' per-lane code on the host.
 * Flattens the scene if needed (no device involved; the scene stays mutable unless committed).
 * Call with out == NULL to get the size.  Offsets are byte offsets into the blob. */
typedef struct hrt_blob_info {
  uint64_t off_nodes, off_prims, off_insts, off_media, off_mats, off_texs, off_perlin, off_images;
  uint32_t n_nodes;        /* node-stream entries: main stream + medium boundary subtrees */
  uint32_t main_end;       /* end of the main stream */
  uint32_t n_prims;
  uint32_t feature_mask;
  uint32_t cull_mode;      /* the default culling (layout.h CULL_*) */
  uint32_t motion_uniform; /* every moving sphere shares time0 / time1 */
  float motion_t0, motion_span;
  float ln_e;
  uint32_t media_nested;   /* a ConstantMedium inside a Translation/Rotation */
  float box_t0, box_t1;    /* ray times the BVH boxes are valid for */
  uint64_t off_walk;       /* sphere scenes: the walk stream of the default (exact) sphere kernel */
  uint32_t walk_bytes;     /* its size (0: not a sphere scene) */
  uint32_t walk_regrouped; /* its inner boxes re-grouped over the reference leaf order */
  uint32_t bvh_tied_sorts; /* as hrt_scene_info */
  uint32_t walk_hot;       /* > 0: the walk stream's first walk_hot bytes are staged in LDS, the rest is read
                            * from global memory (streams beyond the LDS budget) */
  uint32_t walk_general;   /* 1: the walk stream is the general-scene stream (leaf programs, render_gwalk_kernel);
                            * 0: the sphere-scene stream (render_basic_kernel) */
  uint64_t off_chains;     /* every instance's transform chain, outermost first (layout.h CHAIN_F4) */
  uint32_t walk_half;      /* bytes from a walk-stream node part's first 16 B to its second: 16, or the split of
                            * sphere streams staged whole in LDS (layout.h WALK_SPLIT_HALF) */
  uint32_t walk_c16;       /* 1: 16-B node parts (layout.h WALK_C16; hybrid sphere streams): positions are node
                            * indices, the walk ends at walk_nodes, payloads from walk_pbase */
  uint32_t walk_nodes;     /* node parts of the walk stream */
  uint32_t walk_pbase;     /* walk_c16: byte offset of the payloads */
} hrt_blob_info;
hrt_status hrt_debug_scene_blob(hrt_scene* s, void* out, uint64_t cap, uint64_t* size, hrt_blob_info* info);
/* The sample chunks a render of these params would use (no device involved; an uncommitted scene is flattened
 * without its walk streams, which the schedule does not depend on):
 * out[0] = chunk size, out[1] = head chunks, out[2] = samples of the first chunk, out[3] = halving tail chunks.
 * A pixel's samples are summed chunk by chunk and the chunk sums added in chunk order, so this schedule is
 * what fixes the image's bits beyond the paths themselves (hrt_scene_options chunk_*). */
hrt_status hrt_debug_sample_chunks(hrt_scene* s, const hrt_render_params* p, uint32_t* out4);
/* Overwrite n bytes of the committed scene's DEVICE blob at byte `offset` (hrt_blob_info offsets), after
 * a device synchronisation.  Fault injection for the watchdog test (e.g. a skip link pointing back). */
hrt_status hrt_debug_poke_blob(hrt_scene* s, uint64_t offset, const void* data, uint64_t n);
/* The flattened 48-byte record of a primitive (order 0: reference pre-order, 1: SAH streams). */
hrt_status hrt_debug_prim_record(const hrt_scene* s, int32_t order, uint32_t index, float* out12);
/* Evaluate the shared deterministic math on the DEVICE (op: 0 sin, 1 cos, 2 acos, 3 atan2, 4 ln,
 * 5 pow5, 6 tan, 7 the walk's division x / y, 8 / 9 the saturating casts `as i32` / `as u32` with the
 * integer's bits in out) for n inputs; used by the GPU KAT test to prove host/device bit identity. */
hrt_status hrt_debug_device_math(int32_t op, const float* x, const float* y, float* out, uint32_t n);
/* The walk's inflated box test (CULL_EXACT's culling half, lane.h box_ce; form 0: sub/mul/add, 1: the fused
 * o*inv form) on every (box, ray) pair, on the DEVICE (on_device = 1: the calling thread's current HIP device) or with the same code compiled for
 * the host (0): boxes n_boxes x 8 floats (C.xyz, -, E.xyz, -), rays n_rays x 6 floats (origin, direction),
 * out[b * n_rays + q] = 1 if box b passes for ray q on [tmin, tmax].  Used by the GPU test that holds the
 * device's culling decisions to the host's bit for bit. */
hrt_status hrt_debug_box_test(int32_t form, int32_t on_device, const float* boxes, uint32_t n_boxes, const float* rays,
                              uint32_t n_rays, float tmin, float tmax, uint8_t* out);
/* The accumulator's arithmetic (csrc/accum.h) on the DEVICE through the real kernels (on_device = 1: the calling
 * thread's current HIP device) or with the same code compiled for the host (0): partial is one pass's chunk sums
 * [n_chunks][n] x 4 f32, acc_inout the n x 4 f32 sums before and after the pass (w = 0), out the frame of
 * `samples` samples in an HRT_ACCUM_* format after it (format -1: no resolve, out unused).  Used by the tests
 * that check the arithmetic without a GPU and hold the device to the host bit for bit. */
hrt_status hrt_debug_accumulate(int32_t on_device, const float* partial, uint32_t n_chunks, uint32_t n, float* acc_inout,
                                uint64_t samples, int32_t format, void* out);
/* The noise estimate's arithmetic (csrc/accum.h) for ONE tile of n pixels, on the DEVICE through the real kernels
 * (accumulate_chunks with moments, accum_noise; on_device = 1: the calling thread's current HIP device) or with the
 * same code compiled for the host (0): partial is one pass's chunk sums [n_chunks][n] x 4 f32 and sizes its chunks'
 * sample counts; acc_inout (n x 4 f32) and m2_inout (n f32) are the sums and moments before and after the pass;
 * samples = N and chunks = K held after it; err_out takes the n errors and mean_max_out the tile's mean and max. */
hrt_status hrt_debug_noise(int32_t on_device, const float* partial, const uint32_t* sizes, uint32_t n_chunks, uint32_t n,
                           float* acc_inout, float* m2_inout, uint64_t samples, uint64_t chunks, float floor, float* err_out,
                           float* mean_max_out);
/* hrt_accum_add_paths' arithmetic (csrc/accum_paths.h) for n_px pixels of `samples` paths each, packed pixel-major, with
 * the same code compiled for the host (on_device = 0; no device involved) or through the real kernel on one
 * identity-mapped tile (1: the calling thread's current HIP device).  sched3 = (chunk, head chunks, samples of the first
 * chunk), the first three words of hrt_debug_sample_chunks; it must cut [0, samples) into chunks.  acc_inout (n_px x 4 f32)
 * and m2_inout (n_px f32, or NULL: no noise plane) are the sums and moments before and after the pass; out the frame of
 * total_samples samples in an HRT_ACCUM_* format after it (format -1: none), which on the device must equal accum_resolve
 * of the same sums; *live_out (may be NULL) takes the number of records that are not HRT_PATH_DONE. */
hrt_status hrt_debug_accum_paths(int32_t on_device, const hrt_path* paths, uint32_t n_px, uint32_t samples, const uint32_t* sched3,
                                 float* acc_inout, float* m2_inout, uint64_t total_samples, int32_t format, void* out,
                                 uint32_t* live_out);
/* The noise plane of a HRT_ACCUM_NOISE accumulator (n_pixels f32, packed as the tiles are) into host memory, after a
 * device synchronisation: for the tests that hold m2 to its bit contract. */
hrt_status hrt_debug_accum_moments(hrt_accum* a, float* m2_out);
/* The filter's iterations (csrc/filter.h) on a raster the caller gives, on the DEVICE through filter_atrous
 * (on_device = 1: the calling thread's current HIP device) or with the same arithmetic on the host (0).
 * raster: width x height x 4 f32 (c.xyz, v; v < 0: absent); out: width x height x 4 f32 (c'.xyz BEFORE the sqrt, v');
 * an absent pixel comes out as it went in.  1 <= width, height <= 65535. */
hrt_status hrt_debug_filter(int32_t on_device, const float* raster, uint32_t width, uint32_t height, uint32_t iterations,
                            float sigma, float* out);
/* hrt_debug_filter for the guided filter (csrc/filter.h): albedo and normal are the two feature rasters, width x
 * height x 4 f32 ((a.xyz, -) and (n.xyz, z)), read at present pixels only; kn, ka, kz are the terms' 1 / tolerance
 * (0: off; negative or NaN: HRT_ERR_INVALID_ARG). */
hrt_status hrt_debug_guided(int32_t on_device, const float* raster, const float* albedo, const float* normal, uint32_t width,
                            uint32_t height, uint32_t iterations, float sigma, float kn, float ka, float kz, float* out);
/* hrt_debug_guided with hrt_guided_ex_params' flags and albedo_floor (the same checks).  With HRT_GUIDED_DEMODULATE
 * the raster is already gather's (c, v): steps 2 to 4 of the demodulated frame's contract run on it, the divisor from
 * the albedo raster, and out is (c''.xyz BEFORE the sqrt, v' in demodulated units); an absent pixel comes out as it
 * went in.  flags == 0: hrt_debug_guided. */
hrt_status hrt_debug_guided_ex(int32_t on_device, const float* raster, const float* albedo, const float* normal, uint32_t width,
                               uint32_t height, uint32_t iterations, float sigma, float kn, float ka, float kz, uint32_t flags,
                               float albedo_floor, float* out);
/* hrt_accum_noise_filtered's arithmetic on a raster the caller gives (hrt_debug_guided_ex's arguments and checks; the
 * raster is gather's (c, v)), cut into `tiles`, which lie inside the raster, do not overlap and cover present pixels
 * only (HRT_ERR_INVALID_ARG otherwise): on the DEVICE through the real last-iteration and reduce kernels (on_device = 1)
 * or with the same arithmetic on the host (0).  err_out takes the errs packed as the tiles are (the sum of w * h
 * floats), mean_max_out n_tiles x (mean, max).  floor as hrt_accum_noise_filtered's.  With kn = ka = kz = 0 and
 * flags == 0 the feature rasters are not read and may be NULL. */
hrt_status hrt_debug_noise_filtered(int32_t on_device, const float* raster, const float* albedo, const float* normal, uint32_t width,
                                    uint32_t height, uint32_t iterations, float sigma, float kn, float ka, float kz, uint32_t flags,
                                    float albedo_floor, float floor, const hrt_tile* tiles, uint32_t n_tiles, float* err_out,
                                    float* mean_max_out);
/* The raw feature sums (fa, fn) of a HRT_ACCUM_FEATURES accumulator (n_pixels x 4 f32 each, packed as the tiles are)
 * into host memory, after a device synchronisation: for the tests that hold the planes to their bit contract. */
hrt_status hrt_debug_accum_features(hrt_accum* a, float* fa_out, float* fn_out);
/* One builder of the sphere walk stream's hierarchy on n bare leaf boxes (n x 6 floats: min
 * xyz, max xyz), the code commit runs: builder 0 the host's greedy split, 1 the host's DP over 2 x half area, 2 the
 * host's DP over half area x leaves, 3 the greedy split with the DP (1) on ranges of at most dp_sub leaves, 4 the
 * device build on the calling thread's current HIP device.  Writes the 2n - 1 nodes in pre-order: leaf[i] the leaf
 * index or -1 for an inner node, end[i], depth[i], node_boxes 6 floats per node.  A box that is not finite or has
 * min > max, n == 0, and n > 2048 for builders 1 and 2 are HRT_ERR_INVALID_ARG, and nothing is written.  Used by
 * the tests that hold the builders to a restatement of their cut rules and the device build to the host's. */
hrt_status hrt_debug_walk_regroup(int32_t builder, const float* boxes, uint32_t n, uint32_t dp_sub, int32_t* leaf,
                                  uint32_t* end, uint32_t* depth, float* node_boxes);

#ifdef __cplusplus
}
#endif
#endif /* HRT_HRT_H */
