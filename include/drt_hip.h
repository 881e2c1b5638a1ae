/*
 * drt_hip.h -- C ABI of libdrt_hip.so: the MI355X (gfx950) wavefront replacement for the
 * per-pixel forward integrator + reverse-mode gradient accumulator of
 * thalesfm/differentiable-renderer.
 *
 * What each entry point replaces in the reference (all paths relative to /root/reference):
 *
 *   drt_hip_upload_scene    the scene block of src/render.cpp:26-59 (parameters, materials,
 *                           shapes, Scene vector) flattened to POD records; plugin types are
 *                           include/drt/shape.hpp:37-111 (Plane, Sphere),
 *                           include/drt/bxdf.hpp:56-124 (DiffuseBxDF, SpecularBxDF),
 *                           include/drt/emitter.hpp:15-25 (AreaEmitter).
 *   drt_hip_update_params   re-assigning the Vector<T,3,true> scene parameters
 *                           (src/render.cpp:26-29) between optimisation steps.
 *   drt_hip_render          the pixel x sample loop src/render.cpp:72-86: Camera::sample
 *                           (include/drt/camera.hpp:51-60) -> Pathtracer::trace
 *                           (include/drt/pathtracer.hpp:121-136) -> radiance.detach() /
 *                           radiance.backward(g) (include/drt/vector.hpp:256-284), with the
 *                           gradient accumulator VariableNode::backward
 *                           (include/drt/vector.hpp:185-188) as out_param_grad.
 *
 * Conventions: every function returns 0 on success or a negative drt_status; nothing throws
 * across the ABI; the caller owns every host buffer; the context owns device memory and its
 * stream; a context is not thread-safe; calls are synchronous unless DRT_RENDER_DEVICE_OUT is
 * set (then outputs are device pointers, written on the context's stream, and the call returns
 * after enqueueing unless DRT_RENDER_SYNC is also set; the path kernels of consecutive such frames
 * may run side by side on streams of the context's own -- the outputs are still written in the
 * order of the context's stream, and a device adjoint image is read in that order too).
 *
 *   drt_hip_create_group    the same path on SEVERAL GPUs of one node from one process (SURVEY 8b:
 *   drt_hip_comm_init_rank  "ctx owns device memory/streams/RCCL comms"): the rows of the frame are
 *                           dealt to the devices in interleaved bands, every device runs the whole
 *                           pipeline on its bands, and the ONE cross-device step is the reduction of
 *                           the gradient accumulator VariableNode::backward's `m_grad += grad`
 *                           (include/drt/vector.hpp:185-188): one ncclAllReduce(sum, f64, P x 3) over
 *                           xGMI, enqueued by the library on the context's stream after K7.
 *                           create_group = one process, n devices; comm_init_rank = one process per
 *                           GPU (the launcher broadcasts the 128-byte id out of band).
 *
 *   drt_hip_pin_host        nothing in the reference (its image is a `new Vector<double,3>[W*H]` the loop writes in place,
 *                           src/render.cpp:66,82): lets the device do the same -- write the frame straight into the caller's
 *                           buffer -- for callers that render frame after frame.
 *
 * There is NO CPU fallback behind this ABI: without a HIP device drt_hip_create fails with
 * DRT_ERR_NO_DEVICE.
 */
#ifndef DRT_HIP_H
#define DRT_HIP_H

#if defined(__HIPCC_RTC__)
/* compiled by hiprtc at run time (the library specialises k_path for a scene: csrc/drt_jit.h): no system headers there */
typedef signed char int8_t; typedef unsigned char uint8_t; typedef short int16_t; typedef unsigned short uint16_t;
typedef int int32_t; typedef unsigned int uint32_t; typedef long long int64_t; typedef unsigned long long uint64_t;
typedef unsigned long size_t;
#else
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define DRT_HIP_ABI_VERSION 8

typedef enum drt_status {
    DRT_OK = 0,
    DRT_ERR_INVALID = -1,     /* bad argument / malformed scene */
    DRT_ERR_NO_DEVICE = -2,   /* no HIP device / device id out of range */
    DRT_ERR_HIP = -3,         /* a HIP runtime call failed, see drt_hip_last_error */
    DRT_ERR_NO_SCENE = -4,    /* render before upload_scene */
    DRT_ERR_OOM = -5,         /* device allocation failed */
    DRT_ERR_UNSUPPORTED = -6, /* the request is outside what the device path covers (see drt_hip_last_error) */
    DRT_ERR_COMM = -7         /* an RCCL call failed, see drt_hip_last_error */
} drt_status;

/* ---- scene description (host-side POD, doubles: the reference computes in double,
 *      src/render.cpp:22; the device converts to its compute type) ------------------------ */

enum { DRT_SHAPE_PLANE = 0, DRT_SHAPE_SPHERE = 1, DRT_SHAPE_MESH = 2,
       DRT_SHAPE_USER = 3 /* a shape of a caller-defined KIND (drt_shape_kind_desc): any analytic Shape<T> subclass,
                             shape.hpp:11-35 -- `mesh` = index into drt_scene_desc.kinds */ };
enum { DRT_BXDF_DIFFUSE = 0, DRT_BXDF_SPECULAR = 1,
       DRT_BXDF_MIRROR = 2 /* bxdf.hpp:126-144 repaired: f = 1/cos, dir = reflect(dir_in, n), pdf 1; param = -1;
                              its sample discards two draws (see drt_rng_u31) */,
       DRT_BXDF_USER = 3   /* DRT_BXDF_USER + k: a BxDF of the caller-defined kind k (drt_bxdf_kind_desc): any other subclass of
                              BxDF<T>, bxdf.hpp:12-25, whose value is colour x a scalar lobe */ };

typedef struct drt_shape_desc {
    int32_t type;      /* DRT_SHAPE_* */
    int32_t material;  /* index into materials, -1 = no BxDF (shape.hpp:26-27 returns nullptr) */
    int32_t emitter;   /* index into emitters,  -1 = no emitter (shape.hpp:29-30) */
    int32_t mesh;      /* MESH: index into meshes; otherwise ignored */
    double p[4];       /* PLANE: normal.xyz (NOT normalised, shape.hpp:58-59), offset
                          SPHERE: center.xyz, radius   MESH: unused
                          USER: values 0..3 of the shape's record (4..7: drt_scene_desc.user_params) */
} drt_shape_desc;

/* A caller-defined analytic shape (ABI v8): what a subclass of the reference's Shape<T> plugin interface (shape.hpp:11-35:
 * virtual intersect(orig, dir, double& t) and normal(point)) becomes on the device.  The two function BODIES are HIP source,
 * compiled at run time (hiprtc) into the scene's own path kernel next to the library's plane and sphere tests:
 *     template <typename R> bool intersect(const R* p, V3<R> o, V3<R> d, R& t) { <intersect_src> }
 *     template <typename R> V3<R> normal(const R* p, V3<R> P)                  { <normal_src> }
 * p = the shape's record of 8 values (drt_shape_desc.p + user_params), o / d = ray origin and (unit) direction, P = the hit
 * point; R is float or double (DRT_RENDER_F64).  Available: V3<R> with .x .y .z and + - * (component-wise, and by a scalar),
 * mk<R>(x, y, z), dot, cross, normalize, sqrt_r, rsqrt_r, div_r, abs_r, min_r, max_r, fma_r (csrc/drt_device.h).  `intersect`
 * returns whether the ray hits at a t > 0 it stores (the contract of shape.hpp:49-56); the closest hit over all shapes and the
 * first-shape-wins tie rule stay the library's (pathtracer.hpp:72-89).  At most DRT_MAX_USER_KINDS kinds per scene.  Scenes
 * with such shapes render on the one-launch path kernels (analytic scenes, any number of parameters, biased and unbiased
 * operator); a context that may not compile (drt_hip_set_specialisation(-1 / 0)) and scenes that also hold a mesh answer
 * DRT_ERR_UNSUPPORTED. */
#define DRT_MAX_USER_KINDS 2
typedef struct drt_shape_kind_desc {
    const char* name;            /* for messages (and for test checkers that know the kind by name) */
    const char* intersect_src;
    const char* normal_src;
} drt_shape_kind_desc;

/* Triangle mesh: an EXTENSION behind the Shape<T> plugin surface (the reference has no
 * triangles).  A MESH shape stands for its triangles listed in index order at
 * the shape's position in the scene, each one a Shape<T> with these semantics (pinned by the
 * brute-force `Triangle : drt::Shape<double>` of oracle/ref_harness.cpp, compiled against the
 * reference headers): two-sided Moller-Trumbore with e1 = v1 - v0, e2 = v2 - v0, hit iff t > 0
 * (the predicate of shape.hpp:55), normal = normalize(cross(e1, e2)), never flipped (like
 * Sphere, shape.hpp:105-106); on exact ties the earlier triangle wins (pathtracer.hpp:80). */
typedef struct drt_mesh_desc {
    int32_t n_vertices, n_triangles;
    const double* vertices;        /* n_vertices x 3 */
    const uint32_t* indices;       /* n_triangles x 3 */
    const int32_t* face_material;  /* n_triangles material indices, or NULL: the shape's material */
    const int32_t* face_param;     /* n_triangles colour-parameter indices, or NULL.  A face with an entry >= 0 has a BxDF of its
                                      own -- type and exponent of the face's material, colour = that parameter: the reference's
                                      `Triangle(..., std::make_shared<DiffuseBxDF<T>>(albedo_of_this_face))` per face, 50,880
                                      albedos for BASELINE config 4's mesh without 50,880 material records; -1 = the material's
                                      own colour.  (A face without material has no BxDF; a mirror has no colour.) */
} drt_mesh_desc;

typedef struct drt_material_desc {
    int32_t type;      /* DRT_BXDF_* */
    int32_t param;     /* index of the colour parameter (bxdf.hpp:82,122 m_color); MIRROR: -1 */
    double exponent;   /* SPECULAR only (bxdf.hpp:123), not differentiable.  USER: value 0 of the BxDF's record (value 1:
                          drt_scene_desc.user_bxdf_params) */
} drt_material_desc;

/* A caller-defined BxDF (ABI v8): what a subclass of the reference's BxDF<T> plugin interface (bxdf.hpp:12-25: sample(normal,
 * dir_in) -> (dir_out, pdf) and operator()(normal, dir_in, dir_out) -> f) becomes on the device, for BxDFs of the form
 * f = colour parameter x scalar (all of the reference's are).  ONE body, HIP source, compiled at run time into the scene's path kernel:
 *     template <typename R> void bxdf(const R* p, V3<R> n, V3<R> d, R u1, R u2, V3<R>& wo, R& pdf, R& bs) { <sample_src> }
 * p = the BxDF's record of 2 values, n = the surface normal as the shape returns it, d = the direction of the ARRIVING ray
 * (dir_in = -d), u1 / u2 = the two uniform draws sample() consumes, in its order (every BxDF of this build consumes exactly two:
 * drt_rng_u31); out: wo = the sampled direction, pdf = its density, bs = the scalar with f(n, -d, wo) = colour x bs.  Also
 * available: make_frame(n, t, b), sincospi_r(x, &s, &c), pow_r, sqrt_r (csrc/drt_device.h).  Same limits as caller-defined shapes. */
#define DRT_MAX_USER_BXDF_KINDS 2
typedef struct drt_bxdf_kind_desc {
    const char* name;
    const char* sample_src;
} drt_bxdf_kind_desc;

typedef struct drt_emitter_desc {
    int32_t param;     /* index of the emission parameter (emitter.hpp:24) */
    int32_t reserved;
} drt_emitter_desc;

typedef struct drt_scene_desc {
    int32_t n_shapes, n_materials, n_emitters, n_params;
    const drt_shape_desc* shapes;        /* order = Scene order: first shape wins ties,
                                            pathtracer.hpp:80 */
    const drt_material_desc* materials;
    const drt_emitter_desc* emitters;
    const double* params;                /* n_params x 3 (RGB) */
    const uint8_t* requires_grad;        /* n_params, NULL = all true */
    int32_t n_meshes;
    int32_t n_kinds;                     /* (ABI <= 7: reserved, 0) caller-defined shape kinds; -1: none, but caller-defined BxDF kinds
                                            below (n_bxdf_kinds is read); 0: none of the fields behind `meshes` is read */
    const drt_mesh_desc* meshes;
    const drt_shape_kind_desc* kinds;    /* n_kinds */
    const double* user_params;           /* n_shapes x 4: values 4..7 of every shape's record (read for USER shapes only), or NULL: zeros */
    int32_t n_bxdf_kinds, reserved2;     /* caller-defined BxDF kinds; 0: the fields below are not read (n_kinds == 0 too: neither are these) */
    const drt_bxdf_kind_desc* bxdf_kinds;
    const double* user_bxdf_params;      /* n_materials: value 1 of every material's record (read for USER BxDFs only), or NULL: zeros */
} drt_scene_desc;

typedef struct drt_camera_desc {
    int32_t width, height;
    double vfov;                          /* camera.hpp:15 default 1.3963 */
    double eye[3], forward[3], right[3], up[3];   /* as stored by Camera / look_at,
                                                     camera.hpp:29-37 */
} drt_camera_desc;

/* render flags */
#define DRT_RENDER_BACKWARD   0x1u  /* also run the tape backward pass -> out_param_grad */
#define DRT_RENDER_DEVICE_OUT 0x2u  /* out_rgb / out_param_grad / adjoint are DEVICE pointers */
#define DRT_RENDER_SYNC       0x4u  /* with DEVICE_OUT: synchronise the stream before return */
#define DRT_RENDER_TIMING     0x8u  /* bracket every kernel launch with HIP events -> stats */
#define DRT_RENDER_F64        0x10u /* compute in double on the device (verification mode) */
#define DRT_RENDER_ALLREDUCE  0x40u /* with BACKWARD, on a context that has a communicator (drt_hip_comm_init_rank):
                                       after K7 the library enqueues ONE ncclAllReduce(sum, f64, n_params x 3) on
                                       the context's stream; out_param_grad is the sum over ALL ranks' shards.
                                       Every rank of the communicator must make the call.  (A group context
                                       always reduces; the flag is implied.) */
#define DRT_RENDER_ALLREDUCE_ASYNC 0x80u /* like DRT_RENDER_ALLREDUCE, for renders with DRT_RENDER_DEVICE_OUT that follow each other
                                       without a wait in between: the all-reduce and the copy of the reduced gradient into
                                       out_param_grad are enqueued on a SECOND stream of the context and overlap the next render's
                                       kernels (the ~30-60 us of an xGMI all-reduce of 96 bytes would otherwise stand between two
                                       0.85 ms frames on every rank).  out_param_grad is valid after drt_hip_synchronize(ctx) (or
                                       with DRT_RENDER_SYNC), NOT in the order of drt_hip_stream(ctx).  Alternate between two
                                       out_param_grad buffers if every frame's gradient is wanted.  Without DRT_RENDER_DEVICE_OUT
                                       the flag means DRT_RENDER_ALLREDUCE (drt_hip_render_async overlaps its all-reduce anyway). */
#define DRT_RENDER_SERIAL     0x100u /* with DEVICE_OUT: this frame's path kernel does not overlap its neighbours' -- everything of the frame runs
                                       on the context's stream, in order.  What an optimisation loop gets, whose frame i + 1 needs the
                                       gradients of frame i (README.md:88-101); bench.py's `serial_frame`. */
#define DRT_RENDER_LOSS_L2    0x400u /* with BACKWARD: a loss that is NOT linear in the radiance, per SAMPLE -- the reference's loop
                                       `loss = loss_func(radiance); loss.backward()` (README.md:93-98) with loss_func = squared error:
                                       adjoint_rgb is read as a TARGET image (required), and every camera sample s of pixel p is
                                       back-propagated with the seed d|L_s - target_p|^2 / dL_s = 2 (L_s - target_p) instead of a
                                       per-pixel constant.  out_param_grad = d/d params of the sum over all samples of |L_s - target|^2.
                                       (The per-pixel adjoint_rgb of the default mode is exact for losses on the pixel MEAN.)
                                       Biased operator, summed gradients (not with DRT_RENDER_UNBIASED or the gradient image). */
#define DRT_RENDER_UNFUSED    0x200u /* scenes of analytic shapes: the textbook wavefront -- K1 raygen, then per bounce K2 (k_intersect) and K3
                                       (k_shade) as launches of their own over the ray queues in HBM -- instead of the fused routes
                                       (measurement / cross-check: the paths of bounces_per_launch >= 1, values equal to f32 rounding) */
#define DRT_RENDER_UNBIASED   0x20u /* with BACKWARD: the reference's unbiased integration operator
                                       (integrate.hpp:39-52, README.md:104-136): backward draws a
                                       FRESH direction at every vertex and traces a new suffix path
                                       (O(depth^2) segments).  Draw positions follow the reference
                                       with zero-length rays never hitting (oracle/ref_harness.cpp). */

typedef struct drt_render_params {
    int32_t spp;            /* samples per pixel            (args.hpp:36-43, -n) */
    int32_t min_bounces;    /* Pathtracer ctor              (args.hpp:44-51, -b) */
    double absorb;          /* Pathtracer ctor              (args.hpp:52-59, -p) */
    int32_t max_depth;      /* extension: hard cap on path vertices, 1..DRT_MAX_DEPTH; <=0 = DRT_MAX_DEPTH.
                               The reference has none (termination by roulette only): paths the cap cuts
                               short are reported in drt_hip_stats.capped_paths, so the bias is visible.
                               With absorb == 1 the cap is min_bounces itself (every path ends there). */
    uint32_t seed;          /* key of the counter RNG, see drt_rng_u31 */
    int32_t shard, n_shards, band_rows;  /* pixel sharding: image rows are cut into bands of
                               band_rows rows dealt round-robin to n_shards; this call renders
                               the bands of `shard`. n_shards <= 1 renders everything. */
    uint32_t flags;         /* DRT_RENDER_* */
    int64_t batch_paths;    /* paths in flight per wavefront batch, <=0 = default: the largest power of two whose
                             * buffers (~0.2 KB per path) fit in an eighth of the device's memory, at most 32 GB */
    int32_t bounces_per_launch; /* scenes of analytic shapes: bounces a shade launch takes a ray through in
                               registers before survivors are compacted back into the queue (1 = the
                               classic one-launch-per-bounce wavefront, HBM-bound; up to 8). <= 0 = automatic:
                               analytic scenes with at most 8 parameters take the whole path in ONE launch, in
                               registers (k_path, DRT_K_PATH: same samples, sums in another order -- equal to f32
                               rounding); otherwise as many bounces per launch as most rays are expected to survive.
                               Values >= 1 give bitwise identical results among themselves. */
    int32_t reserved;
} drt_render_params;

#define DRT_MAX_DEPTH 64

enum {
    DRT_K_RAYGEN = 0,    /* K1 */
    DRT_K_INTERSECT = 1, /* K2 */
    DRT_K_SHADE = 2,     /* K3 (+ K4 compaction fused: ballot/prefix-sum queue append) */
    DRT_K_FILM = 3,      /* K5 */
    DRT_K_BACKWARD = 4,  /* K6 */
    DRT_K_GRADREDUCE = 5,/* K7 */
    DRT_K_INTERSECT_MESH = 6, /* K2 on triangles: the BVH walk (k_intersect_mesh), timed apart from K2's analytic pass */
    DRT_K_PATH = 7,      /* K1+K2+K3+K6 in ONE launch (k_path): a path lives in registers from the eye to its end */
    DRT_K_COUNT = 8
};

typedef struct drt_hip_stats {
    uint64_t paths;                 /* camera samples traced by this call */
    uint64_t segments;              /* ray segments = raycast calls, camera ray included,
                                       zero-direction continuations excluded */
    uint64_t batches;
    double ms_total;                /* wall time of the call (host clock) */
    double ms_kernel[DRT_K_COUNT];  /* summed HIP-event time per kernel (DRT_RENDER_TIMING) */
    uint64_t launches[DRT_K_COUNT];
    uint64_t units[DRT_K_COUNT];    /* work items processed: paths (K1, K5), segments (K3, K6, k_path), rays tested by
                                       k_intersect (mesh scenes: the camera rays only), candidate rays walked by
                                       k_intersect_mesh (the rays that reach the bounds of the mesh) */
    uint64_t queue_rays_read;       /* rays the shade launches read from the queue (a fused launch keeps a ray */
    uint64_t queue_rays_written;    /* in registers over several bounces) / survivors they wrote back: 32 B each */
    uint64_t capped_paths;          /* paths still alive when they reached max_depth (cut short: 0 when the cap is
                                       the roulette's own certain kill, absorb == 1 at min_bounces); under
                                       DRT_RENDER_UNBIASED every walk counts, the camera paths' and the suffixes'.
                                       Without a user max_depth the limit is DRT_MAX_DEPTH and a path whose roulette
                                       ends it AT that depth is not cut short: its draw is consumed as the reference
                                       consumes it, and with capped_paths == 0 the render is the reference's */
    uint64_t bvh_bytes;             /* mesh scenes: bytes of the BVH (nodes + triangle records) the walk reads from */
    uint64_t path_bytes;            /* k_path launches: the bytes they write (per-range pixel sums, per-block gradient
                                       partials, per-wave counters) -- everything that kernel moves through HBM */
    uint32_t path_program;          /* k_path launches: which closest-hit program ran (DRT_PROGRAM_*; same results, different cost) */
    uint32_t reserved;
    double jit_ms;                  /* host time this context has spent compiling and loading specialised programs so far */
} drt_hip_stats;

/* k_path's closest-hit program (Pathtracer::raycast, pathtracer.hpp:72-89, over the analytic shapes) */
enum {
    DRT_PROGRAM_NONE = 0,        /* the render did not go through k_path */
    DRT_PROGRAM_SORTED = 1,      /* shape kinds read at run time: records sorted by kind in LDS, one counted loop per kind */
    DRT_PROGRAM_BUILTIN = 2,     /* kinds compiled in, the instantiation the library carries for the reference's own scene (render.cpp:39-47) */
    DRT_PROGRAM_SPECIALISED = 3  /* kinds compiled in at run time for THIS scene (hiprtc; drt_hip_set_specialisation) */
};

typedef struct drt_hip_ctx drt_hip_ctx;

int drt_hip_abi_version(void);
int drt_hip_device_count(void);
int drt_hip_create(int device_id, drt_hip_ctx** out);
/* One process, n GPUs.  The group context owns one member context per entry of device_ids
 * (device memory, stream) and the RCCL communicators between the distinct devices (ncclCommInitAll).
 * upload_scene / update_params go to every member; drt_hip_render renders member i's interleaved
 * row bands on device_ids[i] -- all members enqueued before any is waited for -- and returns the whole
 * frame in out_rgb and the gradient ALREADY summed over the members in out_param_grad: members that
 * share a device are added on that device, the distinct devices by ONE ncclAllReduce.  Host buffers only
 * (DRT_RENDER_DEVICE_OUT is refused); rp->shard / n_shards address the GROUP as one shard of a larger job
 * (multi-node), normally 0 / 1.  A device may be listed more than once (testing on a single-GPU box). */
int drt_hip_create_group(const int* device_ids, int n_devices, drt_hip_ctx** out);
int drt_hip_group_size(const drt_hip_ctx* ctx);   /* members of a group context, 1 for a plain one */
/* The PCI bus id ("0000:c1:00.0") of the device member `member` of the context renders on (0 for a plain context): what a
 * launcher logs to show that N ranks -- or the N members of a group -- really sit on N different GPUs. */
int drt_hip_device_pci_bus_id(const drt_hip_ctx* ctx, int member, char* out, int capacity);
void drt_hip_destroy(drt_hip_ctx* ctx);
/* One process per GPU: rank 0 calls drt_hip_comm_unique_id and hands the 128 bytes to the other ranks
 * out of band (torch.distributed store, MPI, a file); every rank then calls drt_hip_comm_init_rank on its
 * own context (collective: returns when all n_ranks have joined).  From then on a render with
 * DRT_RENDER_BACKWARD | DRT_RENDER_ALLREDUCE returns gradients summed over all ranks. */
#define DRT_HIP_UNIQUE_ID_BYTES 128
typedef struct drt_hip_unique_id { char bytes[DRT_HIP_UNIQUE_ID_BYTES]; } drt_hip_unique_id;   /* = ncclUniqueId */
int drt_hip_comm_unique_id(drt_hip_unique_id* out);
int drt_hip_comm_init_rank(drt_hip_ctx* ctx, const drt_hip_unique_id* id, int rank, int n_ranks);
int drt_hip_comm_size(const drt_hip_ctx* ctx);    /* ranks of the context's communicator, 0 = none */
int drt_hip_comm_destroy(drt_hip_ctx* ctx);
int drt_hip_upload_scene(drt_hip_ctx* ctx, const drt_scene_desc* scene);
int drt_hip_update_params(drt_hip_ctx* ctx, const double* params /* n_params x 3 */);
/* When a scene of analytic shapes gets a path kernel compiled for ITS shape kinds (the reference dispatches
 * Shape::intersect through a vtable per shape and ray, shape.hpp:11-35; the device wants the kinds as compile-time
 * constants: ~25 % faster than reading them at run time).  The library carries that kernel for the reference's own scene;
 * for any other it compiles one with hiprtc (~0.5 s of host time per kernel variant, cached per process), bit-identical
 * in its results to the run-time program it replaces:
 *   DRT_SPECIALISE_GENERIC the run-time program even for the reference's own scene (measurement: what specialisation buys)
 *   DRT_SPECIALISE_NEVER   never compile at run time (the reference's own scene keeps the kernel the library carries for it)
 *   DRT_SPECIALISE_AUTO    (default) once the scene has rendered 2^31 path-bounces through this context (~20 ms of
 *                          frames): small test frames never pay for a compile, a render loop does within its first frames
 *                          -- on a thread of the library's own: no frame waits for the compiler, the frames rendered
 *                          meanwhile use the run-time program (drt_hip_stats.path_program says which one ran).  The
 *                          per-sample loss (DRT_RENDER_LOSS_L2) on the one-launch route is a kernel of this kind too: its
 *                          compile starts with the first such frame, the tape route renders until it has delivered
 *   DRT_SPECIALISE_NOW     at the next render that can use it, which waits for the compile (a caller that knows it
 *                          will render many frames and wants every one of them on the fast kernel)
 * The environment variable DRT_HIP_JIT (-1 | 0 | 1 | force) sets the default of new contexts.  Group contexts: every member. */
enum { DRT_SPECIALISE_GENERIC = -1, DRT_SPECIALISE_NEVER = 0, DRT_SPECIALISE_AUTO = 1, DRT_SPECIALISE_NOW = 2 };
int drt_hip_set_specialisation(drt_hip_ctx* ctx, int mode);
/* out_rgb: width*height*3 floats, row-major, mean over spp; only the rows of this shard are
 *          written (others untouched). May be NULL.
 * adjoint_rgb: width*height*3 floats, the seed every sample of that pixel is back-propagated
 *          with; NULL = all ones (src/render.cpp:80 `radiance.backward(Vec3(1))`).
 * out_param_grad: n_params*3 doubles, SUM over this shard's samples (the caller adds it to its
 *          accumulator like vector.hpp:187 does; across shards: one sum all-reduce). */
int drt_hip_render(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp,
                   const float* adjoint_rgb, float* out_rgb, double* out_param_grad,
                   drt_hip_stats* stats);
/* A caller that renders frame after frame into the SAME host buffers (the loop of src/render.cpp:72-90 inside an optimisation
 * loop) can hand them to the context once: drt_hip_pin_host page-locks [ptr, ptr + bytes) and maps it into the device's
 * address space (hipHostRegister), and every later render whose out_rgb (or out_grad_rgb) lies inside a pinned range gets its
 * image written THERE by the finishing kernel -- no staging block, no memcpy at the end of the call (config 3: 3 MB per
 * frame).  The range must stay allocated until drt_hip_unpin_host(ptr) or drt_hip_destroy; results are bit-identical.
 * Plain contexts (a group context's members render into their own staging blocks). */
int drt_hip_pin_host(drt_hip_ctx* ctx, void* ptr, size_t bytes);
int drt_hip_unpin_host(drt_hip_ctx* ctx, void* ptr);
#define DRT_HIP_FRAMES_IN_FLIGHT 4

/* The same call WITHOUT the wait at its end, for callers that render frame after frame (the loop of src/render.cpp:72-90
 * inside an optimisation loop): drt_hip_render_async enqueues the frame and returns a ticket; the results travel to a
 * pinned block of the context on a second stream while the NEXT frame's kernels run, and drt_hip_wait(ticket) hands them
 * to out_rgb / out_param_grad (plain memcpy) and fills `stats` (totals only; no per-kernel times).  Buffer lifetime: out_rgb,
 * out_param_grad must stay valid until drt_hip_wait returns -- they are written THERE, by the calling thread; adjoint_rgb is
 * consumed before drt_hip_render_async returns.  At most DRT_HIP_FRAMES_IN_FLIGHT (four) frames are in flight (one more
 * drt_hip_render_async before the oldest was waited for returns DRT_ERR_INVALID; with three or four in flight the path
 * kernels of consecutive frames overlap), tickets are waited for in order of issue, and drt_hip_render /
 * drt_hip_render_gradient_image refuse to run while frames are in flight.  Host buffers only; a plain (non-group) context.
 * Results are bit-identical to drt_hip_render's. */
int drt_hip_render_async(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp,
                         const float* adjoint_rgb, float* out_rgb, double* out_param_grad, uint64_t* ticket);
int drt_hip_wait(drt_hip_ctx* ctx, uint64_t ticket, drt_hip_stats* stats /* may be NULL */);
/* Per-pixel gradient image (the figure of the reference's README.md:142-145): like drt_hip_render
 * with DRT_RENDER_BACKWARD, but instead of one summed gradient vector it returns
 *   out_grad_rgb[pixel] = mean over the pixel's samples of d(seed . radiance) / d params[param]
 * (the 3 channels of that one parameter), i.e. what `param.grad()` holds after back-propagating
 * only this pixel's samples, divided by spp.  out_rgb may be NULL. */
int drt_hip_render_gradient_image(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp,
                                  int32_t param, const float* adjoint_rgb, float* out_rgb,
                                  float* out_grad_rgb, drt_hip_stats* stats);
/* Forward mode (the reference's Dual<T>, include/drt/dual.hpp, run through the path tracer): the image AND its derivative
 * along ONE direction of parameter space, the Jacobian-vector product J v --
 *   out_tangent_rgb[pixel] = mean over the pixel's samples of d radiance / d eps at params + eps * param_tangent
 * (3 channels; param_tangent: n_params x 3, one direction per parameter value).  One render whatever n_params is; no seed, no
 * accumulator: it shares nothing with the reverse mode but the paths, and <J v, w> = <v, J^T w> ties the two together
 * (spp * sum_pixels w . out_tangent_rgb = sum_params out_param_grad(adjoint = w) . param_tangent).
 * Conventions of drt_hip_render_gradient_image: only this shard's rows of either image are written; out_rgb may be NULL; host
 * buffers (pinned ranges are written directly) or device pointers with DRT_RENDER_DEVICE_OUT; DRT_RENDER_TIMING, _F64, _SERIAL;
 * refused (DRT_ERR_INVALID) while asynchronous frames are in flight.  requires_grad is a reverse-mode notion and is ignored.
 * DRT_ERR_INVALID: NULL param_tangent or out_tangent_rgb, a tangent value that is not finite, DRT_RENDER_BACKWARD, _UNBIASED,
 * _LOSS_L2 or _ALLREDUCE* in rp->flags.  DRT_ERR_UNSUPPORTED (the message says "tangent"): a scene that holds a triangle mesh,
 * bounces_per_launch >= 1, DRT_RENDER_UNFUSED -- the tangent image comes from the one-launch path kernel of analytic scenes
 * (caller-defined kinds included) --, and a GROUP context: render the shards on plain contexts.
 * Geometry, camera and exponents are not differentiable on the device, in either mode. */
int drt_hip_render_tangent(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp,
                           const double* param_tangent /* n_params x 3 */, float* out_rgb /* may be NULL */,
                           float* out_tangent_rgb, drt_hip_stats* stats);
/* ... with both images in double, as the device summed them (a float holds 7 digits; the DRT_RENDER_F64 verification mode is
 * good for 1e-9: this is what a Dual<double> render is compared through).  Host buffers only (DRT_RENDER_DEVICE_OUT:
 * DRT_ERR_INVALID), synchronous; everything else as above. */
int drt_hip_render_tangent_double(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp,
                                  const double* param_tangent, double* out_rgb /* may be NULL */,
                                  double* out_tangent_rgb, drt_hip_stats* stats);
/* The Gauss-Newton normal equations of a frame, and on request its whole Jacobian image, from ONE render.  With P = n_params and
 *   J[x,p,ch] = what drt_hip_render_tangent returns at pixel x, channel ch, along the direction that is 1 on the three channels of
 *               parameter p and 0 elsewhere (same camera, same rp); 0 for a parameter with requires_grad == 0
 * -- a radiance channel depends on the same channel of every parameter only, so J is block-diagonal by channel -- the call returns
 *   out_A[ch][p][q] = sum_x J[x,p,ch] J[x,q,ch]   (3 x P x P doubles, symmetric, both triangles written)
 *   out_b[ch][p]    = sum_x J[x,p,ch] r[x,ch]     (3 x P)
 *   out_loss[ch]    = sum_x r[x,ch]^2             (3, may be NULL)
 * summed over the pixels of this call's shard (the caller adds shards), in fp64, without atomics: the same call returns the same bits.
 * Exactly one of target_rgb and residual_rgb (H x W x 3 floats) is given: with target_rgb, r = this render's own pixel means - target --
 * one render per step, but J and r then share their samples and b is biased (tools/fit_albedo.py says by how much); with residual_rgb,
 * r is the caller's, e.g. from an independently seeded forward render, and out_b is what drt_hip_render returns as out_param_grad / spp
 * for that adjoint.  out_jacobian (P x H x W x 3 floats, may be NULL) receives the P images drt_hip_render_gradient_image returns one
 * at a time; out_rgb may be NULL; of both only this shard's rows are written.  DRT_RENDER_DEVICE_OUT: every image-sized pointer and
 * out_A, out_b, out_loss are device pointers, written in the order of drt_hip_stream().  DRT_RENDER_F64, _SYNC, _TIMING (k_normal_eq is
 * counted in the gradient reduction's slot) and shards as in drt_hip_render_tangent.
 * Roulette-terminated renders are allowed, but a lane of the path kernel is a pixel here, so they run in lockstep: every wave lasts as
 * long as the longest of its 64 paths, where the regenerating form drt_hip_render takes for such renders keeps its lanes busy (the
 * reference's defaults, -b 1 -p 0.5: 0.87 against 0.50 ms on a 512 x 512 x 64 frame).
 * DRT_ERR_UNSUPPORTED (the message says "normal equations"): more than DRT_FAST_PARAMS (8) parameters -- drt_hip_render_normal_equations_along
 * (8 directions per render) or J^T J v by tangent + reverse are the routes for those; a mirror material costs one of the 8 columns (its internal colour constant), so a scene with a
 * mirror may have 7 --, more than 2^31 camera samples in the frame (the shard renders in one batch; batch_paths is ignored), a render
 * that a DRT_HIP_* setting forces onto the queue wavefront or into several batches, a scene that holds a triangle mesh, bounces_per_launch >= 1, DRT_RENDER_UNFUSED, _UNBIASED,
 * _LOSS_L2, _ALLREDUCE, _ALLREDUCE_ASYNC, a group context.  DRT_ERR_INVALID: both or neither of target_rgb and residual_rgb, NULL
 * out_A or out_b, a value of a host image that is not finite, asynchronous frames in flight.  The context stays usable after either. */
int drt_hip_render_normal_equations(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp,
                                    const float* target_rgb /* or NULL */, const float* residual_rgb /* or NULL */,
                                    float* out_rgb /* may be NULL */, double* out_A /* 3 x P x P */, double* out_b /* 3 x P */,
                                    double* out_loss /* 3, may be NULL */, float* out_jacobian /* P x H x W x 3, may be NULL */,
                                    drt_hip_stats* stats);
/* J v_k for k < n_dirs directions of parameter space in ONE render: out_tangents[k] (H x W x 3 floats each) is what
 * drt_hip_render_tangent returns for param_tangents[k] (n_params x 3 doubles each) -- the same path, the same sums per direction, for any
 * number of scene parameters the path kernels stage (136): the forward mode keeps one running sum per direction and channel and no
 * per-parameter state.  1 <= n_dirs <= DRT_HIP_MAX_DIRS; the kernel is instantiated for 2, 4 and 8 directions and a call's count is
 * padded up with zero directions, which add exact zeros: the image of a direction depends neither on the other directions nor on n_dirs,
 * bit for bit.  With V = unit vectors of a block of parameters this is the Jacobian image of a P-parameter scene in ceil(P / 8) renders;
 * with V = the columns of d theta / d phi it is the Jacobian of a reparametrised scene (one tint over ten albedos; albedo = s base).
 * Rules of drt_hip_render_normal_equations for everything but the directions (shards, DRT_RENDER_DEVICE_OUT -- out_rgb and out_tangents
 * are then device pointers; the directions are host memory always --, _F64, _SYNC, _TIMING, one batch, lockstep under the roulette);
 * rules of drt_hip_render_tangent for the directions (finite values, requires_grad ignored).  With DRT_RENDER_F64 the float images are
 * the double sums rounded.
 * DRT_ERR_INVALID: n_dirs outside 1 ... DRT_HIP_MAX_DIRS, NULL param_tangents or out_tangents, a direction value that is not finite,
 * asynchronous frames in flight.  DRT_ERR_UNSUPPORTED: a scene that holds a triangle mesh, bounces_per_launch >= 1, DRT_RENDER_UNFUSED,
 * _UNBIASED, _LOSS_L2, _ALLREDUCE*, a group context, more than 136 parameters, a render forced into several batches or onto the queue
 * wavefront.  The message of either says "tangents"; the context stays usable. */
#define DRT_HIP_MAX_DIRS 8
int drt_hip_render_tangents(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_dirs,
                            const double* param_tangents /* n_dirs x n_params x 3 */, float* out_rgb /* may be NULL */,
                            float* out_tangents /* n_dirs x H x W x 3 */, drt_hip_stats* stats);
/* ... and the normal equations in their span -- Gauss-Newton / Levenberg-Marquardt over span(V), exact for a reparametrised scene,
 * for scenes of any number of parameters (drt_hip_render_normal_equations stops at 8).  With T[x,k,ch] = out_tangents[k][x][ch]:
 *   out_A[ch][k][l] = sum_x T[x,k,ch] T[x,l,ch]   (3 x K x K doubles, K = n_dirs, both triangles written)
 *   out_b[ch][k]    = sum_x T[x,k,ch] r[x,ch]     (3 x K)
 *   out_loss[ch]    = sum_x r[x,ch]^2             (3, may be NULL)
 * from the same render, reduced by the kernels of drt_hip_render_normal_equations (fp64, no atomics: the same call returns the same
 * bits; the sums are over this call's shard).  Exactly one of target_rgb and residual_rgb, as there; out_tangents may be NULL.
 * Refusals as above plus DRT_ERR_INVALID for both or neither of target_rgb and residual_rgb, NULL out_A or out_b and a value of a host
 * image that is not finite; the message says "normal equations along". */
int drt_hip_render_normal_equations_along(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_dirs,
                                          const double* param_tangents /* n_dirs x n_params x 3 */,
                                          const float* target_rgb /* or NULL */, const float* residual_rgb /* or NULL */,
                                          float* out_rgb /* may be NULL */, double* out_A /* 3 x K x K */, double* out_b /* 3 x K */,
                                          double* out_loss /* 3, may be NULL */, float* out_tangents /* n_dirs x H x W x 3, may be NULL */,
                                          drt_hip_stats* stats);
/* ... with b and the loss UNBIASED from this one render.  drt_hip_render_normal_equations_along with target_rgb forms b = J^T r from pixel
 * means that share their samples with J: per pixel b carries Cov(t_k, L) / n and the loss Var(L) / n (n = spp, t_k = J_s v_k and L per
 * sample), so a fit settles where the NOISY objective has its minimum.  The camera samples of a pixel are independent streams (the RNG
 * contract above), so the mean over ordered pairs s != s' of the pixel's samples -- a U-statistic, all samples used -- has the product of
 * the expectations as its expectation, exactly.  With T_k, m the pixel means, r = m - target, cov and var the SAMPLE covariance and variance:
 *   out_A[ch][k][l]  = sum_x T_k T_l                       (what _along returns: the products of the means.  Its expectation exceeds
 *                                                           mu mu^T by the positive semi-definite Cov / n: damping, which does not move
 *                                                           the point where out_b = 0.  Debiasing A would take K (K + 1) / 2 more moment
 *                                                           rows per channel and is not done)
 *   out_b[ch][k]     = sum_x (T_k r - cov(t_k, L) / n)     = sum_x 1 / (n (n - 1)) sum_{s != s'} t_{k,s} (L_s' - target)
 *   out_loss[ch]     = sum_x (r^2 - var(L) / n)            = sum_x 1 / (n (n - 1)) sum_{s != s'} (L_s - target) (L_s' - target)
 *   out_bias[ch][k]  = sum_x cov(t_k, L) / n  (k < K),  out_bias[ch][K] = sum_x var(L) / n       (3 x (K + 1), may be NULL): what was
 *                      subtracted -- out_b + out_bias and out_loss + out_bias[.][K] are the plain values of _along; out_bias[.][K] is the
 *                      render's own noise floor in the loss
 *   out_variance_rgb[x][ch] = var(L) / n                   (H x W x 3 floats, may be NULL): the variance of the pixel's mean
 * out_rgb and out_tangents (both may be NULL) are what drt_hip_render_tangents returns, bit for bit in the library's kernels.  The path
 * kernel is the K-direction form plus 3 K + 3 fp64 moment sums per lane; k_cross_eq reduces in fp64 without atomics: the same call
 * returns the same bits; the sums are over this call's shard.  1 <= n_dirs <= DRT_HIP_MAX_DIRS_CROSS.  Rules of _along for everything else
 * (shards, DRT_RENDER_DEVICE_OUT -- every pointer but the directions is then a device pointer --, _F64, _SYNC, _TIMING, one batch,
 * lockstep under the roulette, 2^31 samples).
 * DRT_ERR_INVALID: spp < 2 (the estimator needs a pair), NULL target_rgb, out_A, out_b, out_loss or param_tangents, n_dirs outside
 * 1 ... DRT_HIP_MAX_DIRS_CROSS, a value of the directions or of a host target that is not finite, asynchronous frames in flight.
 * DRT_ERR_UNSUPPORTED: whatever _along refuses.  The message says "normal equations cross"; the context stays usable. */
#define DRT_HIP_MAX_DIRS_CROSS 8
int drt_hip_render_normal_equations_cross(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_dirs,
                                          const double* param_tangents /* n_dirs x n_params x 3 */, const float* target_rgb /* H x W x 3 */,
                                          float* out_rgb /* may be NULL */, double* out_A /* 3 x K x K */, double* out_b /* 3 x K */,
                                          double* out_loss /* 3 */, double* out_bias /* 3 x (K + 1), may be NULL */,
                                          float* out_tangents /* n_dirs x H x W x 3, may be NULL */,
                                          float* out_variance_rgb /* H x W x 3, may be NULL */, drt_hip_stats* stats);
/* ONE frame under n_sets parameter vectors in one trace: out_images[k] (H x W x 3 floats) is what drt_hip_update_params(param_sets[k])
 * followed by drt_hip_render returns -- a parameter is a colour or an emission, nothing that decides where a path goes sees its value, so
 * the sets share the ray, the RNG key, the hit and the BxDF sample and each keeps its own throughput and radiance, moved by the forward
 * render's own operations.  With target_rgb,
 *   out_loss[k][ch] = sum over the pixels of this call's shard of (mean_k - target)^2        (n_sets x 3 doubles)
 * reduced in fp64 without atomics: the same call returns the same bits.  A line search, the dampings of a Levenberg-Marquardt step, a
 * finite-difference probe or a population of candidates costs one trace per seed.  1 <= n_sets <= DRT_HIP_MAX_PARAM_SETS; the kernel is
 * instantiated for 2, 4 and 8 sets and a call's count is padded up with copies of the context's own parameters, which are never written
 * out: the image of a set depends neither on its companions nor on n_sets, bit for bit.  A set holds the caller's parameters
 * (n_params x 3 doubles); the colour constant a mirror material appends keeps the scene's own value in every set.  The context's own
 * parameters are not changed.  out_rgb, where given, is the plain image of the context's own parameters from the same trace; it takes
 * one of the kernel's sets, so out_rgb beside 8 sets is refused (DRT_ERR_UNSUPPORTED) -- drt_hip_render gives that image.
 * Shards, DRT_RENDER_DEVICE_OUT (target_rgb, out_images, out_loss and out_rgb are then device pointers; param_sets is host memory
 * always), _F64, _SYNC, _TIMING, one batch per shard, lockstep under the roulette, the 2^31-sample limit: as drt_hip_render_tangents.  The
 * reduction is timed in the gradient-reduction slot of drt_hip_stats.
 * DRT_ERR_INVALID: n_sets outside 1 ... DRT_HIP_MAX_PARAM_SETS, NULL param_sets, a value that is not finite, neither out_images nor
 * out_loss, out_loss without target_rgb, asynchronous frames in flight, DRT_RENDER_BACKWARD.  DRT_ERR_UNSUPPORTED: a scene that holds a
 * triangle mesh, a group context, bounces_per_launch >= 1, DRT_RENDER_UNFUSED, _UNBIASED, _LOSS_L2, _ALLREDUCE*, more than 136
 * parameters, a render forced into several batches or onto the queue wavefront.  The message of either says "param sets"; the context
 * stays usable. */
#define DRT_HIP_MAX_PARAM_SETS 8
int drt_hip_render_param_sets(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_sets,
                              const double* param_sets /* n_sets x n_params x 3 */, const float* target_rgb /* H x W x 3, may be NULL */,
                              float* out_images /* n_sets x H x W x 3, may be NULL */, double* out_loss /* n_sets x 3, may be NULL */,
                              float* out_rgb /* may be NULL */, drt_hip_stats* stats);
/* ... the images as the means the device formed, in double: host buffers only */
int drt_hip_render_param_sets_double(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_sets,
                                     const double* param_sets /* n_sets x n_params x 3 */, const float* target_rgb /* H x W x 3, may be NULL */,
                                     double* out_images /* n_sets x H x W x 3, may be NULL */, double* out_loss /* n_sets x 3, may be NULL */,
                                     float* out_rgb /* may be NULL */, drt_hip_stats* stats);
/* ... each set with a DIRECTION of its own, in one trace: what a strong-Wolfe line search, a cubic step picker or a Levenberg-Marquardt
 * gain ratio needs per candidate P_k -- out_images[k] as above, out_tangents[k] = J(P_k) d_k (what drt_hip_update_params(param_sets[k]) +
 * drt_hip_render_tangent(param_tangents[k]) returns, by the forward-mode form's own operations on set k's operands), and with the residual
 * r_k = mean_k - target over the pixels of this call's shard, n_sets x 3 doubles each,
 *   out_loss[k][ch]  = sum r_k^2          out_dloss[k][ch] = sum 2 r_k (J d_k)          out_curv[k][ch] = sum (J d_k)^2
 * the value, the slope along d_k and the Gauss-Newton curvature of the loss, reduced in fp64 without atomics: the same call returns the
 * same bits.  1 <= n_sets <= DRT_HIP_MAX_SETS_ALONG; the kernel is instantiated for 2 and 4 sets and a call's count is padded up with
 * copies of the context's own parameters and zero directions, which are never written out: a set's results depend neither on its companions
 * nor on n_sets, bit for bit.  A channel of a set that is exactly zero is handled as the forward-mode form handles it.  The colour constant a
 * mirror material appends keeps the scene's own value and a zero tangent in every set.  The context's own parameters are not changed.
 * There is no out_rgb: drt_hip_render gives that image.  out_loss and out_dloss need target_rgb; out_curv does not.  Everything else --
 * shards, DRT_RENDER_DEVICE_OUT (target_rgb and every out_* are then device pointers; param_sets and param_tangents are host memory always),
 * _F64, _SYNC, _TIMING, one batch per shard, lockstep under the roulette, the 2^31-sample limit, the slot the reduction is timed in -- as
 * drt_hip_render_param_sets.
 * DRT_ERR_INVALID: n_sets outside 1 ... DRT_HIP_MAX_SETS_ALONG, NULL param_sets or param_tangents, a value that is not finite, no output
 * requested, out_loss or out_dloss without target_rgb, asynchronous frames in flight, DRT_RENDER_BACKWARD.  DRT_ERR_UNSUPPORTED: what
 * drt_hip_render_param_sets refuses.  The message of either says "param sets along"; the context stays usable. */
#define DRT_HIP_MAX_SETS_ALONG 4
int drt_hip_render_param_sets_along(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_sets,
                                    const double* param_sets /* n_sets x n_params x 3 */, const double* param_tangents /* n_sets x n_params x 3 */,
                                    const float* target_rgb /* H x W x 3, may be NULL */, float* out_images /* n_sets x H x W x 3, may be NULL */,
                                    float* out_tangents /* n_sets x H x W x 3, may be NULL */, double* out_loss /* n_sets x 3, may be NULL */,
                                    double* out_dloss /* n_sets x 3, may be NULL */, double* out_curv /* n_sets x 3, may be NULL */,
                                    drt_hip_stats* stats);
/* ... the images as the means the device formed, in double: host buffers only */
int drt_hip_render_param_sets_along_double(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_sets,
                                           const double* param_sets /* n_sets x n_params x 3 */,
                                           const double* param_tangents /* n_sets x n_params x 3 */,
                                           const float* target_rgb /* H x W x 3, may be NULL */, double* out_images /* n_sets x H x W x 3, may be NULL */,
                                           double* out_tangents /* n_sets x H x W x 3, may be NULL */, double* out_loss /* n_sets x 3, may be NULL */,
                                           double* out_dloss /* n_sets x 3, may be NULL */, double* out_curv /* n_sets x 3, may be NULL */,
                                           drt_hip_stats* stats);
/* ... each set's summed GRADIENT, in one trace: what K Adam chains, the accepted point of a line search, a population of candidates or a
 * finite-difference check need at several points at once.  out_param_grads[k] is what drt_hip_update_params(param_sets[k]) followed by
 * drt_hip_render(DRT_RENDER_BACKWARD, adjoints_rgb[k]) writes to out_param_grad: J(P_k)^T w_k as the SUM over this shard's samples, zeros for
 * parameters with requires_grad == 0.  The sets share the path and its vertex history (neither sees a parameter's value); where the path
 * meets a light every set runs the general gradient form's own code on its own operands, into its own rows of the wave's fp64 table, and
 * k_sets_grad_finish adds the blocks in a fixed order without atomics: the same call returns the same bits.  1 <= n_sets <=
 * DRT_HIP_MAX_SETS_GRAD; the kernel is instantiated for 2, 4 and 8 sets and a call's count is padded up with copies of the context's own
 * parameters, which add nothing: a set's gradient depends neither on its companions nor on its position, and not on n_sets within a width,
 * bit for bit.  The table has 408 elements per wave: width x 3 x (parameters that require a gradient) may not exceed it.  The colour
 * constant a mirror material appends keeps the scene's value in every set and has no output row.  The context's own parameters are not
 * changed.  adjoints_rgb == NULL seeds every pixel of every set with (1, 1, 1), as drt_hip_render does.  DRT_RENDER_BACKWARD is implied and
 * may be set or not.  There are no images in this call: the adjoint exists before the trace, and drt_hip_render_param_sets on the other
 * seed gives the images it comes from.  Everything else -- shards, DRT_RENDER_DEVICE_OUT (adjoints_rgb and out_param_grads are then device
 * pointers; param_sets is host memory always), _F64, _SYNC, _TIMING, one batch per shard, lockstep under the roulette, the 2^31-sample
 * limit, the slot the reduction is timed in -- as drt_hip_render_param_sets.
 * DRT_ERR_INVALID: n_sets outside 1 ... DRT_HIP_MAX_SETS_GRAD, NULL param_sets or out_param_grads, a set or an adjoint value that is not
 * finite (host buffers), asynchronous frames in flight, bad camera or render parameters.  DRT_ERR_UNSUPPORTED: what
 * drt_hip_render_param_sets refuses, and more rows than the table holds.  The message of either says "param sets grad"; the context stays
 * usable. */
#define DRT_HIP_MAX_SETS_GRAD 8
int drt_hip_render_param_sets_grad(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_sets,
                                   const double* param_sets /* n_sets x n_params x 3 */,
                                   const float* adjoints_rgb /* n_sets x H x W x 3, may be NULL */,
                                   double* out_param_grads /* n_sets x n_params x 3 */, drt_hip_stats* stats);
/* ... each set's loss UNBIASED, from the one trace: what an accept / reject, a gain ratio, a line search or a population compares.
 * drt_hip_render_param_sets' loss sum_x (mean_k - target)^2 carries sum_x Var(L_k) / n (n = spp), which depends on the set -- a brighter
 * candidate is noisier --, so the plain losses of two candidates differ by the difference of their noise as well.  Per set k, over the pixels
 * of this shard, with m_k the pixel's mean, r_k = m_k - target and var^ the sample variance of the pixel's n samples under set k:
 *   out_loss[k][ch]         sum_x (r_k^2 - var^(L_k) / n) = sum_x 1 / (n (n - 1)) sum_{s != s'} (L_{k,s} - t)(L_{k,s'} - t): its expectation is
 *                           the loss of the converged images (it may be negative)
 *   out_bias[k][ch]         sum_x var^(L_k) / n, what was subtracted: out_loss + out_bias is drt_hip_render_param_sets' loss
 *   out_variance[k][x][ch]  var^(L_k) / n, the variance of the pixel's mean under set k
 *   out_images[k]           drt_hip_render_param_sets' image k, bit for bit
 * The path kernel is a form of its own (k_path_sets_cross): drt_hip_render_param_sets' operations on the path, plus per lane and set the fp64
 * sums of the samples' squares (exact products of f32 values; raw moments add across sample ranges); k_sets_cross_finish forms the
 * corrections per pixel in fp64 and adds them in a fixed order without atomics: the same call returns the same bits.  1 <= n_sets <=
 * DRT_HIP_MAX_SETS_CROSS; the kernel is instantiated for 2, 4 and 8 sets and a call's count is padded up with copies of the context's own
 * parameters, which are never written out: a set's results depend neither on its companions nor on its position nor on n_sets, bit for bit.
 * The context's own parameters are not changed.  There is no out_rgb and no _double twin.  Everything else -- shards,
 * DRT_RENDER_DEVICE_OUT (target_rgb and the outputs are then device pointers; param_sets is host memory always), _F64, _SYNC, _TIMING, one
 * batch per shard, lockstep under the roulette, the 2^31-sample limit, the slot the reduction is timed in -- as drt_hip_render_param_sets.
 * DRT_ERR_INVALID: spp < 2, NULL target_rgb, out_loss or param_sets, n_sets outside 1 ... DRT_HIP_MAX_SETS_CROSS, a set or a target value
 * that is not finite (host buffers), asynchronous frames in flight, DRT_RENDER_BACKWARD, bad camera or render parameters.
 * DRT_ERR_UNSUPPORTED: what drt_hip_render_param_sets refuses.  The message of either says "param sets cross"; the context stays usable. */
#define DRT_HIP_MAX_SETS_CROSS 8
int drt_hip_render_param_sets_cross(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_sets,
                                    const double* param_sets /* n_sets x n_params x 3 */, const float* target_rgb /* H x W x 3 */,
                                    float* out_images /* n_sets x H x W x 3, may be NULL */, double* out_loss /* n_sets x 3 */,
                                    double* out_bias /* n_sets x 3, may be NULL */, float* out_variance /* n_sets x H x W x 3, may be NULL */,
                                    drt_hip_stats* stats);
/* ---- one scene from up to DRT_HIP_MAX_VIEWS cameras in ONE trace: what a fitting loop over several views of a scene renders per step.  For
 * rp_v = *rp with seed = seeds ? seeds[v] : rp->seed, view v's results are what drt_hip_render(ctx, &cams[v], &rp_v, adjoints_rgb + v H W 3, ...)
 * returns:
 *   out_images[v]      that call's out_rgb, bit for bit, in f32 and under DRT_RENDER_F64
 *   out_view_grads[v]  that call's out_param_grad, bit for bit -- the SUM over this shard's samples, zeros for requires_grad == 0 -- wherever
 *                      drt_hip_render itself runs a lockstep form of the library's kernels: fixed-depth renders, through the built-in or the
 *                      kind-sorted program.  (A roulette-terminated render runs in lockstep here, as in every derived form; drt_hip_render
 *                      takes the regenerating form there, whose f32 sums are other sums of the same terms: equal within the stated f32 bound;
 *                      in f64 the gradients within 1e-9 of the largest component, the images -- floats on both sides -- within 1e-9 of the
 *                      largest value plus one float ulp of it.)
 *   out_param_grad     the views' gradients added in view order in fp64
 * stats->paths, ->segments and ->capped_paths are the sums over the views; launches[DRT_K_PATH] == 1 for any n_views.  The path kernel is a
 * shell of its own (k_path_views): the single frame's grid once per view -- the same samples per wave, every view on a block boundary -- whose
 * blocks take their view's camera constants, seed and stream from a table the host fills per call, and then run the single call's operations on
 * the single call's operands; k_views_finish adds a view's partial sums in the single call's order, and no float is added by an atomic: the same
 * call returns the same bits.  All cameras share width and height.  rp->shard / n_shards / band_rows apply to every view alike, and only the
 * shard's rows of each image are written.  DRT_RENDER_BACKWARD is needed for either gradient output; _F64, _TIMING, _SYNC and _DEVICE_OUT as in
 * drt_hip_render_param_sets_grad (with _DEVICE_OUT adjoints_rgb and the three outputs are device pointers; cams and seeds are host memory
 * always).  One batch per shard, on the context's stream, in order.
 * DRT_ERR_INVALID: n_views outside 1 ... DRT_HIP_MAX_VIEWS, NULL cams or rp, cameras of different sizes, no output requested, a gradient output
 * without DRT_RENDER_BACKWARD (the flag without a gradient output renders forward only), an adjoint value that is not finite (host buffers),
 * asynchronous frames in flight.  DRT_ERR_UNSUPPORTED: a scene that holds a triangle mesh, a group context, bounces_per_launch >= 1, DRT_RENDER_UNFUSED, _UNBIASED,
 * _LOSS_L2 or _ALLREDUCE*, more parameters than the path kernels stage (136), more than 2^31 camera samples over all views, a render that a
 * DRT_HIP_* setting forces onto the queue wavefront or whose paths end at depth 0 (batch_paths and DRT_HIP_BATCH_PATHS cannot force several
 * batches: the shard renders in one whatever they say).  The message of either says "views"; the context stays usable. */
#define DRT_HIP_MAX_VIEWS 64
int drt_hip_render_views(drt_hip_ctx* ctx, const drt_camera_desc* cams /* n_views */, int32_t n_views, const drt_render_params* rp,
                         const uint32_t* seeds /* n_views, NULL: rp->seed for every view */,
                         const float* adjoints_rgb /* n_views x H x W x 3, NULL: all ones */,
                         float* out_images /* n_views x H x W x 3, may be NULL */,
                         double* out_param_grad /* n_params x 3, the sum over the views, may be NULL */,
                         double* out_view_grads /* n_views x n_params x 3, may be NULL */, drt_hip_stats* stats);
/* ---- a caller's batch of pixels from up to DRT_HIP_MAX_VIEWS cameras in ONE trace: what a stochastic fitting loop over several views renders
 * per step (a few thousand pixels drawn across all views), and what an adaptive scheme re-renders (the pixels its variance image calls noisy).
 * Entry e of view v is pixel pixels[e] = y W + x of camera v; the views' lists stand one behind the other, counts[v] entries each.  For
 * rp_v = *rp with seed = seeds ? seeds[v] : rp->seed:
 *   out_rgb[e]         that pixel of the image drt_hip_render(ctx, &cams[v], &rp_v, ...) returns, bit for bit, in f32 and under
 *                      DRT_RENDER_F64, wherever drt_hip_render_views promises the same for a whole image (the RNG key of a camera sample is
 *                      pixel spp + sample: a pixel rendered alone draws what it draws inside its frame); entries keep the caller's order
 *   out_view_grads[v]  J_v^T w_v over view v's entries -- the SUM over the samples, w the entries' adjoints (adjoints_rgb, NULL: all ones) --,
 *                      zeros for requires_grad == 0, all zeros for a view with counts[v] == 0.  A pixel may appear any number of times, in
 *                      one view or in several: every occurrence gets the same radiance and counts once in the gradients, with its own
 *                      adjoint.  Against drt_hip_render with the adjoint image that holds, per pixel, the sum of its entries' adjoints: the
 *                      same paths and per-lane sums, another grouping into waves and blocks -- f64 within 1e-9 of the largest component,
 *                      f32 within the stated bound; the full frame as a list (pixels 0 ... W H - 1 per view) is drt_hip_render_views' grid
 *                      and gives its bits
 *   out_param_grad     the views' vectors added in view order in fp64
 * stats->paths = sum(counts) spp; ->segments and ->capped_paths are summed over all entries; launches[DRT_K_PATH] == 1 for any input.  The
 * path kernel is a shell of its own (k_path_pixels): view v's list is a "frame" of counts[v] pixels -- ceil(counts[v] / 64) waves times the
 * sample ranges the plan picks for a single W x H x spp frame (not re-tuned to the list's length: that is what keeps the single call's
 * operations), every view on a block boundary, a view without entries without blocks.  k_pixels_finish adds the ranges and the views'
 * blocks in fixed orders; no float is added by an atomic: the same call returns the same bits.  DRT_RENDER_BACKWARD is needed for either
 * gradient output; _F64, _TIMING, _SYNC and _DEVICE_OUT as in drt_hip_render_views (with _DEVICE_OUT adjoints_rgb and the three outputs are
 * device pointers; cams, seeds, counts and pixels are host memory always).  One batch, on the context's stream, in order.
 * DRT_ERR_INVALID: n_views outside 1 ... DRT_HIP_MAX_VIEWS, NULL cams, rp, counts or pixels, a negative count, sum(counts) == 0, a pixel
 * >= W H, cameras of different sizes, no output requested, a gradient output without DRT_RENDER_BACKWARD, an adjoint value that is not finite
 * (host buffers), rp->n_shards > 1 (a list is the caller's own split), asynchronous frames in flight.  DRT_ERR_UNSUPPORTED: everything
 * drt_hip_render_views refuses (a triangle mesh, a group context, bounces_per_launch >= 1, DRT_RENDER_UNFUSED, _UNBIASED, _LOSS_L2 or
 * _ALLREDUCE*, more than 136 parameters, a DRT_HIP_* setting that forces the queue wavefront, paths that end at depth 0), and more than 2^31
 * camera samples over all entries.  The message of either says "pixels"; the context stays usable. */
int drt_hip_render_pixels(drt_hip_ctx* ctx, const drt_camera_desc* cams /* n_views, one size */, int32_t n_views, const drt_render_params* rp,
                          const uint32_t* seeds /* n_views, NULL: rp->seed for every view */,
                          const int32_t* counts /* n_views: entries of view v, >= 0 */,
                          const uint32_t* pixels /* sum(counts): y * W + x, the views' lists one behind the other */,
                          const float* adjoints_rgb /* sum(counts) x 3, NULL: all ones */,
                          float* out_rgb /* sum(counts) x 3, may be NULL */,
                          double* out_param_grad /* n_params x 3, the sum over all entries, may be NULL */,
                          double* out_view_grads /* n_views x n_params x 3, may be NULL */, drt_hip_stats* stats);
/* ---- the per-sample loss from the caller's own source, with the loss's value.  The reference's loop is
 *     auto radiance = tracer.trace(scene, orig, dir);  auto loss = loss_func(radiance);  loss.backward();       (README.md:93-98)
 * with loss_func the caller's code; DRT_RENDER_LOSS_L2 is the one loss_func the library carries, and returns no value.  Here the loss is the
 * BODY of
 *     template <typename R> void sample_loss(const R* q, V3<R> L, V3<R> t, R& value, V3<R>& grad) { <loss_src> }
 * L = the radiance of ONE camera sample, t = its pixel of the target image, value = loss_func(L), grad = d value / d L; R is float, or double
 * under DRT_RENDER_F64.  Helpers: those of csrc/drt_device.h (mk, dot, sqrt_r, div_r, abs_r, max_r, ...), as for caller-defined shapes.  q[0 ..
 * DRT_MAX_LOSS_VALUES) are the caller's constants (a Huber delta, an epsilon): DATA -- they reach the kernel as an argument, the compile
 * cache goes by the source alone, and setting the same source with other values compiles nothing.  NULL: the squared error, value =
 * |L - t|^2, grad = 2 (L - t).  The source is compiled by hiprtc at the first render that uses it (~0.3-0.5 s, waited for, cached per
 * process).  `name` appears in messages only, reduced to letters, digits and [ _.-]; it never reaches the generated header.
 * drt_hip_render with DRT_RENDER_LOSS_L2 ignores the context's loss.
 * DRT_ERR_INVALID: NULL loss_src, a value that is not finite.  DRT_ERR_UNSUPPORTED: a group context. */
#define DRT_MAX_LOSS_VALUES 4
typedef struct drt_sample_loss_desc {
    const char* name;                       /* for messages */
    const char* loss_src;                   /* the body of sample_loss */
    double values[DRT_MAX_LOSS_VALUES];     /* q[0..3] */
} drt_sample_loss_desc;
int drt_hip_set_sample_loss(drt_hip_ctx* ctx, const drt_sample_loss_desc* loss /* NULL: squared error */);
/* One render under the context's per-sample loss; backward is implied.
 *   out_param_grad[p][c] = sum over this shard's samples of grad_s[c] dL_s[c] / dtheta[p][c] -- with the default loss what
 *                          drt_hip_render(DRT_RENDER_BACKWARD | DRT_RENDER_LOSS_L2, adjoint_rgb = target_rgb) returns
 *   out_loss             = sum over this shard's samples of value_s; a path that reaches no light counts with L = 0
 *   out_rgb              the plain mean image
 * requires_grad, DRT_RENDER_F64, _TIMING, _SYNC, _DEVICE_OUT (target_rgb and the three outputs are then device pointers), shards and
 * batch_paths as in drt_hip_render; the shards' and batches' gradients and losses add.  The route is DRT_RENDER_LOSS_L2's plan, in f64 wherever
 * in f32: ONE k_path launch -- its LOSS instantiation compiled with the loss, whose two seeds call sample_loss and whose lanes add the
 * samples' values into fp64 sums of their own, one partial per wave -- in analytic scenes where no shape both scatters and emits (lockstep
 * and regenerating forms, columns and the general form); else the tape route (meshes, an emitting scatterer, bounces_per_launch >= 1,
 * min_bounces == 0): k_radiance writes every path's radiance, k_sample_seed -- the kernel compiled from the loss -- turns it into the path's
 * seed in place and adds its value into fp64 partials per block, k_backward_seeded walks the gradients.  k_loss_finish adds the partials in
 * a fixed order.  No atomics on the loss: two identical calls return identical bits.  It never falls back to another loss.
 * DRT_ERR_INVALID (the message says "sample loss"): NULL target_rgb; neither out_param_grad nor out_loss nor out_rgb; a target value that is
 * not finite (host buffers only: with DRT_RENDER_DEVICE_OUT the target is device memory the library does not read on the host, and a value
 * that is not finite there comes back as a loss and gradients that are not finite); asynchronous frames in flight; DRT_RENDER_UNBIASED; DRT_RENDER_ALLREDUCE*.  DRT_ERR_UNSUPPORTED ("sample
 * loss"): a group context; a context that may not compile (drt_hip_set_specialisation(DRT_SPECIALISE_NEVER / _GENERIC)); a body hiprtc
 * rejects -- drt_hip_last_error holds the compiler's log.  The context stays usable after each. */
int drt_hip_render_sample_loss(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp,
                               const float* target_rgb /* H x W x 3 */, float* out_rgb /* may be NULL */,
                               double* out_param_grad /* n_params x 3, may be NULL */,
                               double* out_loss /* 1 double, may be NULL */, drt_hip_stats* stats);
/* stream the context launches on (a hipStream_t), for event timing / interop */
void* drt_hip_stream(drt_hip_ctx* ctx);
int drt_hip_synchronize(drt_hip_ctx* ctx);
const char* drt_hip_last_error(drt_hip_ctx* ctx);
const char* drt_hip_kernel_name(int k);

/* ---- the per-path counter RNG (part of the contract: the oracle, the reference harness and
 *      the device all draw from it) --------------------------------------------------------
 * Replaces drt::random::uniform (include/drt/random.hpp:7-10): the n-th rand() call made while
 * tracing camera sample `path` (= pixel*spp + sample, pixel = y*width + x) returns
 * drt_rng_u31(seed, path, n) in [0, 2^31-1]; uniform = r / 2147483647.0 (RAND_MAX).
 *
 *     draw(seed, path, n) = mix32( mix32( mix32(seed + C (path_hi + 1)) + C (n + 1) ) ^ path_lo ) >> 1
 *
 * A path's key is the 64-bit pair (stream = mix32(seed + C (path_hi + 1)), path_lo): two different paths of a render never
 * share a key -- mix32 is a bijection, so at every draw index the paths of one stream (2^32 of them: path_hi fixed) even
 * get pairwise different 32-bit values -- and no path's sequence is a shifted copy of another's: the draw index enters
 * through its own hash round h(n) = mix32(stream + C (n + 1)), the path through the XOR behind it, so "path b replays
 * path a k draws later" would need h(n) ^ h(n + k) = a ^ b for every n.  (Rounds 1-2 drew mix32(key32 + C (n + 1)) with a
 * 32-bit key per path: keys that differ by a multiple of C gave shifted copies of one sequence, and the 16.7 M paths of
 * config 3 collided outright ~3e4 times in the 2^32 key space.  tests/test_oracle_properties.py scans config 3's paths.)
 * h(n) is the same for every path of a render (the device refuses frames of more than 2^32 camera samples: path_hi = 0),
 * so a wave whose lanes stand at the same draw index computes it once, on the scalar unit. */
#if defined(__HIPCC__)
#define DRT_HD __host__ __device__ static inline
#else
#define DRT_HD static inline
#endif

DRT_HD uint32_t drt_mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

typedef struct drt_rng_key {
    uint32_t stream;   /* mix32(seed + C (path_hi + 1)): shared by all paths with the same high word */
    uint32_t lo;       /* low word of the path index */
} drt_rng_key;

DRT_HD uint32_t drt_rng_stream(uint32_t seed, uint32_t path_hi) { return drt_mix32(seed + 0x9E3779B9u * (path_hi + 1u)); }

DRT_HD drt_rng_key drt_rng_path_key(uint32_t seed, uint64_t path)
{
    drt_rng_key k;
    k.stream = drt_rng_stream(seed, (uint32_t)(path >> 32));
    k.lo = (uint32_t)path;
    return k;
}

/* h(n): the draw index's own hash round (the same for every path of a stream) */
DRT_HD uint32_t drt_rng_index_hash(uint32_t stream, uint32_t n) { return drt_mix32(stream + 0x9E3779B9u * (n + 1u)); }

/* the draw, given h(n) and the path's low word */
DRT_HD uint32_t drt_rng_combine(uint32_t index_hash, uint32_t path_lo) { return drt_mix32(index_hash ^ path_lo) >> 1; }

DRT_HD uint32_t drt_rng_draw(drt_rng_key key, uint32_t n)
{
    return drt_rng_combine(drt_rng_index_hash(key.stream, n), key.lo);
}

DRT_HD uint32_t drt_rng_u31(uint32_t seed, uint64_t path, uint32_t n)
{
    return drt_rng_draw(drt_rng_path_key(seed, path), n);
}

#ifdef __cplusplus
}
#endif
#endif /* DRT_HIP_H */
