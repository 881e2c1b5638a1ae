// drt_path.h -- k_path: K1 + K2 + K3 + K6 of a render in ONE launch (gfx950 / wave64).
//
// For scenes of analytic shapes whose paths end at a fixed depth (`-b D -p 1`, or a small max_depth) nothing
// has to leave the CU between the eye and the end of a path: a lane keeps ONE PIXEL, walks its samples one
// after the other and carries every path in registers --
//     ray (o, d), RNG key                                    Camera::sample, camera.hpp:51-60
//     T_k = prod_{j<k} colour_j m_j   (prefix throughput)    Pathtracer::scatter, pathtracer.hpp:91-115
//     L   = sum_k T_k E_k / p_k       (radiance of the path) Pathtracer::trace,   pathtracer.hpp:121-136
// and, when gradients are wanted (<= 4 parameters, the reference's scene has exactly 4, render.cpp:26-29), the
// TANGENTS of the throughput with respect to every parameter,
//     dT_k/dc_p,  updated per vertex:  dT' = dT * (colour m) + [colour is c_p] T m ,
// so that every emissive vertex adds  g * dT_p * E_k / p_k  to parameter p's gradient and  g * T_k / p_k  to its
// own emission parameter -- the very sums the reference's backward functors (vector.hpp:418-484) and
// VariableNode::backward's `m_grad += grad` (vector.hpp:185-188) produce by walking its graph in reverse; here
// they are accumulated in the order the path is traced, so no tape, no vertex count, no queue and no second
// kernel exist: per PATH the launch moves 0 bytes (per pixel and sample range: 24 bytes of radiance sums).
// The wavefront kernels of drt_kernels.h (queues in HBM, tape + K6) remain the general path: meshes, roulette-
// terminated paths of unbounded length, the unbiased operator, more than 4 parameters, gradient images.
//
// Work split: wave <-> (group of 64 consecutive pixels of the batch, range of `spr` samples); a block is four
// neighbouring groups of one range.  Pixel sums leave as f64 partials per range (summed in range order by
// k_film_parts: bitwise reproducible), gradients as per-block fp64 partials for K7 (fixed order), segment counts
// as one word per wave.
//
// Closest hit, f32: the scene's INTERSECTION PROGRAM (DevScene::prog*, built at upload, scene order kept so the
// first shape wins ties, pathtracer.hpp:80): one record per shape with a kind --
//     general plane   t = (o.n - off) * rcp(-(d.n))                        shape.hpp:49-59
//     axis plane      n = +-e_a exactly:  t = (s off - o_a) * rcp(d_a)      -- bit-identical to the general form
//                     (the products with 0 and +-1 are exact, rcp is odd), 2 instead of 9 VALU and the three
//                     rcp(d_a) are shared by all axis planes of the scene
//     sphere          half-b form of shape.hpp:78-103 (b = 2 b', disc = 4 disc': exact power-of-two scalings)
// The kinds are either read from the scene (the kind-sorted program in LDS: one counted loop per kind) or fixed at compile
// time (template SG, a KindSig: the shape loop fully unrolled, records in scalar registers, no branches at all) -- for
// the reference's own scene in the library, for any other analytic scene by hiprtc at run time (drt_jit.h).
#pragma once

#include "drt_kernels.h"
#ifdef DRT_SAMPLE_LOSS
// the caller's per-sample loss (drt_hip_render_sample_loss): sample_loss<R> and its values; in this build only, the LOSS instantiation's two
// seeds call it, and k_path takes the values and a place for its waves' sums of the samples' values behind its arguments
#include "drt_loss.h"
#endif

#define DRT_DRAW_TABLE (3 * DRT_MAX_DEPTH + 8)     // camera 2 (+1), then per vertex theta, phi and the next depth's roulette

struct PathArgs {
    // frame / sharding
    int32_t W, H, spp;
    int32_t shard, n_shards, band;
    // batch: pixels [p0, p0 + Pb) of the shard, samples [s0, s0 + Sb), cut into ranges of spr samples
    uint32_t Pb, p0, Sb, s0, spr, n_ranges, n_groups;
    // integrator
    int32_t min_bounces, depth_cap, cap_is_roulette, cap_draws;   // (cap_draws: BatchArgs)
    uint32_t rr_threshold, seed, rng_stream;   // rng_stream: drt_rng_stream(seed, 0)
    uint32_t regen_min;             // regenerating form: idle lanes it takes to run the camera code (see k_path)
    uint32_t shade_min, descend_min;   // k_path_mesh (drt_path_mesh.h): lanes it takes to run the vertex step / to keep the node loop going
    int32_t gimg_param;             // >= 0: the lanes' gradient sums of this parameter also leave per pixel (gradient image)
    uint32_t gen_rows, gen_clog2;   // NP = DRT_NP_ANY: rows of the gradient tables (3 per parameter that requires a gradient), log2 of the copies a wave keeps of each
    uint32_t hist_lds, hist_stride; // ... full history words a thread keeps in LDS (the rest: global memory), threads of the grid
    uint32_t gimg_row, pad_gen;     // ... the table row of the gradient image's parameter (NC == 1), DRT_SLOT_NONE: it requires no gradient
    unsigned long long hist_ovf;    // ... the history's global part (uint32_t[words][hist_stride]), 0: none
    double p_rr, inv_p_rr;          // 1 - absorb and its reciprocal (pathtracer.hpp:130)
    // camera
    double eye[3], fwd[3], right[3], up[3];
    double tan_half, aspect, inv_W, inv_H;
    // what the f32 kernels use of the doubles above, cast on the host: a scalar register each instead of a v_cvt_f32_f64 result in a vector one
    // (at the END of the record: the f64 kernels' argument offsets stay what their register allocation was tuned at)
    float p_rr_f, inv_p_rr_f;
    float eye_f[3], fwd_f[3], right_f[3], up_f[3], cs_step_f, ct_step_f;   // (cs = cs0 + u1 cs_step: camera.hpp:53-58 in CameraLane's form)
    // The K-direction forward form (NP = DRT_NP_TANGENT, NC = K): how many of the kernel's K directions are the caller's -- their sums leave
    // the kernel, 3 rows each.  It has no gradient tables, so the count shares the word of gen_rows (no field in the middle of the record,
    // none appended: the f64 kernels' argument offsets stay); read and written through these two only.
    __host__ __device__ uint32_t dirs_out() const { return gen_rows; }
    __host__ __device__ void set_dirs_out(uint32_t n) { gen_rows = n; }
};

__device__ inline uint32_t path_global_pixel(const PathArgs& a, uint32_t lp)
{
    uint32_t ly = lp / (uint32_t)a.W, x = lp - ly * (uint32_t)a.W;
    uint32_t y = ly;
    if (a.n_shards > 1) {
        uint32_t b = ly / (uint32_t)a.band, r = ly - b * (uint32_t)a.band;
        y = (b * (uint32_t)a.n_shards + (uint32_t)a.shard) * (uint32_t)a.band + r;
    }
    return y * (uint32_t)a.W + x;
}

template <typename SG>
__device__ inline HitRec<float> path_closest_hit(const DevScene<float>* __restrict__ sc, const ProgRecs<SG::n>& recs, float4 ra, float2 rb)
{
    return closest_hit_prog<SG>(sc, recs, mk<float>(ra.x, ra.y, ra.z), mk<float>(ra.w, rb.x, rb.y));
}
template <typename SG>
__device__ inline HitRec<double> path_closest_hit(const DevScene<double>* __restrict__ sc, const ProgRecs<SG::n, double>& recs, double4 ra, double2 rb)
{
    if (SG::n > 0)                                                 // a compiled-in program in f64
        return closest_hit_sig<SG, double>(recs, mk<double>(ra.x, ra.y, ra.z), mk<double>(ra.w, rb.x, rb.y));
    const double4 ra1[1] = {ra};
    const double2 rb1[1] = {rb};
    HitRec<double> h1[1];
    closest_hit_n<double, 1>(sc, sc->n_shapes, ra1, rb1, h1);      // any other scene: the literal loop
    return h1[0];
}

// the kinds of the reference's scene (render.cpp:39-47): sphere, sphere, -x, general (1, 0, 0.1), -z, +z, +y, -y, sphere
#define DRT_SIG_CORNELL                                                                                                   \
    ((unsigned long long)DRT_PK_SPHERE | (unsigned long long)DRT_PK_SPHERE << 3 | (unsigned long long)DRT_PK_AX << 6 |    \
     (unsigned long long)DRT_PK_PLANE << 9 | (unsigned long long)DRT_PK_AZ << 12 | (unsigned long long)DRT_PK_AZ << 15 |  \
     (unsigned long long)DRT_PK_AY << 18 | (unsigned long long)DRT_PK_AY << 21 | (unsigned long long)DRT_PK_SPHERE << 24)
#define DRT_NSIG_CORNELL 9
typedef KindSig<DRT_SIG_CORNELL, 0ull, 0ull, 0ull, DRT_NSIG_CORNELL> SigCornell;
// ... and its pure lights (an emitter, no BxDF) as a bit set in scene order: the last sphere (k_path_lean's LIGHTS)
#ifndef DRT_LEAN_LIGHTS
#define DRT_LEAN_LIGHTS 1               // the host hands k_path_lean the scene's light set (0: never, the last vertex as it was; the per-part A/B of profiles/r17_path_ends.txt)
#endif
#define DRT_LIGHTS_CORNELL (DRT_LEAN_LIGHTS != 0 ? 1ull << 8 : 0ull)
#ifndef DRT_LEAN_PEEL_LAST
#ifdef DRT_USER_SHAPES
#define DRT_LEAN_PEEL_LAST 0            // (caller-defined kinds: the compiler contracts the caller's inlined intersect body as its surroundings suggest -- written any other
                                        //  way than k_path's loop one pixel of tests/test_gpu_param_sets.py differed by 6.6e-9 from k_path's kernel: the loop's text stays)
#else
#define DRT_LEAN_PEEL_LAST 1            // k_path_lean's last vertex stands behind the bounce loop (0: a test inside the loop, as it was: profiles/r17_path_ends.txt)
#endif
#endif
#ifndef DRT_LEAN_LIVE_MASK
#define DRT_LEAN_LIVE_MASK 1            // k_path_lean's gradient form carries "the lane's path goes on" round its loop as the wave's mask in a scalar pair (0: as a bool; profiles/r18_bounce_fusions.txt)
#endif
#ifndef DRT_LEAN_FOLD_DRAWS
#ifdef DRT_USER_SHAPES
#define DRT_LEAN_FOLD_DRAWS 0           // (caller-defined kinds: the loop's text stays, as above)
#else
#define DRT_LEAN_FOLD_DRAWS 1           // k_path_lean beside a compiled-in program folds the key once per sample and h(n) on the scalar unit (drt_fold.h; 0: the plain draw; profiles/r26_folded_draws.txt)
#endif
#endif

// (DRT_PATH_LDS_PARAMS, drt_device.h: parameters staged in LDS; more: read from L2)

// the part of the scene a vertex of the one-launch kernels needs, compact (SceneLds carries the whole DevScene and 256
// parameters: 10.4 KB; this is 5.2 KB in f32 -- a block per CU more for the regenerating k_path)
template <typename R>
struct PathSceneLds {
    struct {
        int n_shapes, n_materials, n_emitters, n_params;
        DevShape<R> shapes[DRT_MAX_SHAPES];
        DevMaterial<R> materials[DRT_MAX_MATERIALS];
        int emitter_param[DRT_MAX_EMITTERS];
        int flat[DRT_MAX_SHAPES];
    } sc;
    R params[DRT_PATH_LDS_PARAMS * 3];
#ifdef DRT_USER_SHAPES
    R user_q[DRT_MAX_SHAPES][4];           // caller-defined shapes: values 4..7 of their records (the normal needs the whole record)
#endif
};

template <typename R, bool ALL_LDS = false>
__device__ inline V3<R> load_param(const PathSceneLds<R>& lds, const R* __restrict__ params, int id)
{
    if (ALL_LDS || id < DRT_PATH_LDS_PARAMS)
        return mk<R>(lds.params[id * 3], lds.params[id * 3 + 1], lds.params[id * 3 + 2]);
    return mk<R>(params[id * 3], params[id * 3 + 1], params[id * 3 + 2]);
}
// ... of ONE parameter set (NP = DRT_NP_SETS_GRAD): the set's raw values, 3 per parameter, where add_emission's general branch reads a light's
// emission -- handed to it in the scene's place, so the branch runs as it is on the set's own operands
template <typename R>
struct SetParams {
    const R* p;
};
template <typename R, bool ALL_LDS = false>
__device__ inline V3<R> load_param(const SetParams<R>& set, const R* __restrict__, int id)
{
    return mk<R>(set.p[id * 3], set.p[id * 3 + 1], set.p[id * 3 + 2]);
}

template <typename R>
__device__ inline void stage_path_scene(PathSceneLds<R>& lds, const DevScene<R>* __restrict__ sc, const R* __restrict__ params)
{
    const int ns = sc->n_shapes, nm = sc->n_materials, ne = sc->n_emitters;
    if (threadIdx.x < 4)
        reinterpret_cast<int*>(&lds.sc)[threadIdx.x] = reinterpret_cast<const int*>(sc)[threadIdx.x];
    {
        const int* src = reinterpret_cast<const int*>(sc->shapes);
        int* dst = reinterpret_cast<int*>(lds.sc.shapes);
        for (int i = threadIdx.x; i < ns * (int)(sizeof(DevShape<R>) / sizeof(int)); i += blockDim.x)
            dst[i] = src[i];
    }
    {
        const int* src = reinterpret_cast<const int*>(sc->materials);
        int* dst = reinterpret_cast<int*>(lds.sc.materials);
        for (int i = threadIdx.x; i < nm * (int)(sizeof(DevMaterial<R>) / sizeof(int)); i += blockDim.x)
            dst[i] = src[i];
    }
    for (int i = threadIdx.x; i < ne; i += blockDim.x)
        lds.sc.emitter_param[i] = sc->emitter_param[i];
    for (int i = threadIdx.x; i < ns; i += blockDim.x)
        lds.sc.flat[i] = sc->flat[i];
#ifdef DRT_USER_SHAPES
    for (int i = threadIdx.x; i < ns * 4; i += blockDim.x)
        lds.user_q[i >> 2][i & 3] = sc->user_q[i >> 2][i & 3];
#endif
    const int np = sc->n_params < DRT_PATH_LDS_PARAMS ? sc->n_params : DRT_PATH_LDS_PARAMS;
    for (int i = threadIdx.x; i < np * 3; i += blockDim.x)
        lds.params[i] = params[i];
    __syncthreads();
}


// per-lane gradient state: NP parameters (0 = none), of which only the first NC can be a BxDF's colour (the others are
// emission-only parameters: the reference's scene has three albedos and one emission, render.cpp:26-29).
//
// The throughput is a PRODUCT, T = prod_j colour_{p_j} m_j, so its tangent with respect to a colour parameter needs no
// per-vertex update at all (rounds 2-3 carried dT/dc_p per parameter and moved it with 9 fma + 9 selects per bounce):
//     dT_ch / dc_{p,ch} = T_ch n_p / c_{p,ch} ,      n_p = how many vertices of the path scattered on colour p
// -- one 8-bit counter per parameter (a path has at most DRT_MAX_DEPTH = 64 vertices), one packed add per bounce.  A colour
// channel that is ZERO (the reference's red = (0.5, 0, 0), render.cpp:26) has no quotient: the lane's T therefore leaves the
// zero factors out (they are replaced by 1: `colnz`) and counts them per channel instead (`zc`, 8 bits each):
//     T_real,ch       = zc_ch == 0 ? T_ch : 0
//     dT_ch/dc_{p,ch} = c_{p,ch} != 0 ? T_real,ch n_p / c_{p,ch}
//                                     : (n_p == 1 and zc_ch == 1 ? T_ch : 0)     (d/dc of c^n at 0: 1 for n = 1, else 0)
// Evaluated where a path meets a light: once per sample.  Same sums as the reference's backward functors
// (vector.hpp:418-484) in closed form; the image is unchanged bit for bit (a channel without zero factors sees the very
// same multiplications), gradients to f32 rounding.  |c| < DRT_ZERO_CHANNEL = 1e-18 counts as zero (its quotient would overflow).
// Row DRT_TANGENT_REST is for a lane whose path does NOT go on from the vertex: colour (1, 1, 1), increments 0.  The lockstep kernel
// freezes such a lane by pointing its table index there (the index is a select anyway) and its multiplicand m_k at 1: T * (1 * 1) and
// counters + 0 are exact, so the lane keeps its bits -- one select on the index and one on m_k instead of three on the factor and one per counter.
#define DRT_TANGENT_REST DRT_FAST_PARAMS
// The zero-channel rule of every table below, once: |c| < DRT_ZERO_CHANNEL counts as zero, and a table entry (c, v) -- a colour channel and
// its tangent -- splits into the colour with zero replaced by 1, v / c (0 at a zero), v where the channel is zero (else 0), and the zero bit
// (the three values go straight to their table words, in this order: the staging prologues keep their instruction streams).
#define DRT_ZERO_CHANNEL 1e-18
template <typename R>
__device__ inline bool zero_channel(R c) { return abs_r(c) < R(DRT_ZERO_CHANNEL); }
template <typename R>
__device__ inline bool zero_split(R c, R v, R& colnz, R& dlog, R& dzero)
{
    const bool zero = zero_channel(c);
    colnz = zero ? R(1) : c;
    dlog = zero ? R(0) : v / c;
    dzero = zero ? v : R(0);
    return zero;
}
#ifndef DRT_FREEZE_BY_ROW
#define DRT_FREEZE_BY_ROW 1
#endif
template <typename R>
struct TangentLds {              // per colour parameter, wave-uniform except where indexed by the lane's colour id
    R colnz[DRT_FAST_PARAMS + (DRT_FREEZE_BY_ROW != 0)][4];     // the colour with zero channels replaced by 1
    R invc[DRT_FAST_PARAMS][4];          // 1 / c per channel, 0 where the channel is zero
    uint32_t inc[DRT_FAST_PARAMS + (DRT_FREEZE_BY_ROW != 0)][4];   // counter increments of a bounce on this colour: n_p (low, high word), zc; [3] = zero-channel bits
};

template <typename R, typename SL>
__device__ inline void stage_tangents(TangentLds<R>& tl, const SL& lds)
{
    // (after stage_scene's barrier; parameters beyond the scene's own read as (1, 1, 1))
    if (threadIdx.x < DRT_FAST_PARAMS) {
        const int p = threadIdx.x;
        const bool in = p < lds.sc.n_params;
        uint32_t zinc = 0, zbits = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const R c = in ? lds.params[p * 3 + ch] : R(1);
            const bool zero = zero_channel(c);
            tl.colnz[p][ch] = zero ? R(1) : c;
            tl.invc[p][ch] = zero ? R(0) : R(1) / c;
            zinc |= zero ? 1u << (8 * ch) : 0u;
            zbits |= zero ? 1u << ch : 0u;
        }
        tl.colnz[p][3] = R(0);
        tl.invc[p][3] = R(0);
        tl.inc[p][0] = p < 4 ? 1u << (8 * p) : 0u;
        tl.inc[p][1] = p >= 4 ? 1u << (8 * (p - 4)) : 0u;
        tl.inc[p][2] = zinc;
        tl.inc[p][3] = zbits;
    }
    if (DRT_FREEZE_BY_ROW != 0 && threadIdx.x >= DRT_WAVE && threadIdx.x < DRT_WAVE + 4) {
        tl.colnz[DRT_TANGENT_REST][threadIdx.x - DRT_WAVE] = R(1);
        tl.inc[DRT_TANGENT_REST][threadIdx.x - DRT_WAVE] = 0u;
    }
    __syncthreads();
}

// ---- k_path_lean's bounce tables (compiled-in program; profiles/r18_bounce_fusions.txt) -----------------------------------
// What a bounce reads of the shape it hit and of the colour it scattered on, laid out so that ONE register -- the index shifted
// -- addresses every read of a record through the instruction's own offset, and the reads are wide:
//   rec[s]   32 B per shape: (n.xyz | c.xyz, type) -- one ds_read_b128 -- and (the colour row's byte offset, the emission id) -- one
//            ds_read_b64.  DevShape's own record took a shift, two adds, three reads and the split of `pad`.  rec[NS] is the MISS
//            record, where the closest hit's index starts (closest_hit_sig: MISS): neither BxDF nor emitter, so "hit" needs no
//            test and the index no clamp.  Without colour columns (NC == 0) the row offset is the colour id itself.
//   col[r]   32 B per colour: (colnz.xyz, n_p increment low) -- one ds_read_b128 -- and (zc increment, n_p increment high).  Row 0 is
//            TangentLds's rest row (1, 1, 1), zeros; colour p stands in row p + 1.  A lane that goes on selects its record's offset,
//            any other lane 0: no shift, no add.  The same values as TangentLds's colnz / inc, copied, not recomputed.
// Per-lane special cases of k_path_lean's bounce (LEAN_REC) under the lane mask instead of computed for all 64 lanes and kept by select
// (profiles/r27_masked_lanes.txt).  Each switch: bit 0 the gradient forms (NP > 0), bit 1 the forward-only form; 0: the selects, as it was.
//   DRT_LEAN_MASK_NORMAL  the sphere's normal only in the lanes that hit a sphere, behind a branch a wave of plane hits skips (71 % of
//                         config 3's waves at the first vertex, 8 % at the second): both forms;
//   DRT_LEAN_REC_OFFSET   the closest hit hands back the record's byte offset in LeanLds::rec (closest_hit_sig: SCALE), no shift: the
//                         gradient form (forward only: no run-to-run gain over the masked normal alone);
//   DRT_LEAN_MASK_REST    the colour's row, T, n_p and zc only in the lanes whose path goes on -- the rest row's factor is exactly 1
//                         and its increments 0, so a lane that stops keeps the bits it had: the gradient form (forward only: three
//                         instructions shorter and 0.4 % SLOWER, as a shorter loop was in r17 and r18).
#ifndef DRT_LEAN_MASK_NORMAL
#define DRT_LEAN_MASK_NORMAL 3
#endif
#ifndef DRT_LEAN_REC_OFFSET
#define DRT_LEAN_REC_OFFSET 1
#endif
#ifndef DRT_LEAN_MASK_REST
#define DRT_LEAN_MASK_REST 1
#endif
constexpr bool lean_part(int part, int np) { return ((part >> (np == 0 ? 1 : 0)) & 1) != 0; }
#ifndef DRT_LEAN_REC
#define DRT_LEAN_REC 1                  // 0: the bounce reads DevShape and TangentLds as before (the per-part A/B of profiles/r18_bounce_fusions.txt)
#endif
struct alignas(16) LeanRec {
    float4 a;                  // p[0..2], type (bits)
    uint2 b;                   // colour row offset (DRT_ID_NONE: no BxDF), emission id
    uint2 pad;
};
struct alignas(16) LeanCol {
    float4 a;                  // colnz[0..2], inc[0] (bits)
    uint2 b;                   // inc[2], inc[1]
    uint2 pad;
};
template <int NS, int NC>
struct alignas(16) LeanLds {
    LeanRec rec[NS + 1];
    LeanCol col[NC > 0 ? DRT_FAST_PARAMS + 1 : 1];
};
template <typename SG, int NC, bool BY_ROW, bool FIXED, bool NO_LIT_BXDF, bool SPEC, typename R>
constexpr bool lean_rec()
{
#ifdef DRT_USER_SHAPES
    return false;
#else
    return DRT_LEAN_REC != 0 && SG::n > 0 && FIXED && NO_LIT_BXDF && !SPEC && sizeof(R) == 4 && (NC == 0 || BY_ROW);
#endif
}
template <int NS, int NC, typename SL>
__device__ inline void stage_lean(LeanLds<NS, NC>& ll, const SL& lds, const TangentLds<float>& tl)
{
    // (after stage_path_scene's and stage_tangents' barriers: the colour rows are TangentLds's own words)
    if (threadIdx.x <= NS) {
        const int s = threadIdx.x;
        const bool in = s < NS;
        const DevShape<float>& sh = lds.sc.shapes[in ? s : 0];
        const uint32_t ids = in ? (uint32_t)sh.pad : 0xFFFFFFFFu;
        const uint32_t cid = ids & 0xFFFFu, eid = ids >> 16;
        const uint32_t row = NC > 0 ? ((cid < DRT_FAST_PARAMS ? cid : DRT_FAST_PARAMS - 1u) + 1u) * (uint32_t)sizeof(LeanCol) : cid;
        ll.rec[s].a = make_float4(sh.p[0], sh.p[1], sh.p[2], __int_as_float(in ? sh.type : -1));   // (the miss record: shape 0's values, of which nothing is used)
        ll.rec[s].b = make_uint2(cid == DRT_ID_NONE ? DRT_ID_NONE : row, eid);
    }
    if (NC > 0 && threadIdx.x >= DRT_WAVE && threadIdx.x < DRT_WAVE + DRT_FAST_PARAMS + 1) {
        const int r = (int)threadIdx.x - DRT_WAVE;              // row 0: the rest row, row p + 1: colour p
        const int t = r == 0 ? DRT_TANGENT_REST : r - 1;
        ll.col[r].a = make_float4(tl.colnz[t][0], tl.colnz[t][1], tl.colnz[t][2], __uint_as_float(tl.inc[t][0]));
        ll.col[r].b = make_uint2(tl.inc[t][2], tl.inc[t][1]);
    }
    __syncthreads();
}

template <typename R, int NP, int NC>
struct Tangents {
    uint32_t cnt[NC > 4 ? 2 : 1];   // n_p of the current path, 8 bits per colour parameter
    uint32_t zc;                    // zero factors met per channel, 8 bits each
    // The lane's gradient sums, NP x 3 values, live in an LDS column of the block (acc[row][thread]: conflict-free), not
    // in registers: they are touched once per SAMPLE (where the path meets a light), and twelve registers held across the
    // bounce loop cost the kernel its sixth wave per SIMD (96 -> 80 VGPRs; as scratch spills, which is what the compiler
    // makes of them when told to fit six waves, 0.728 -> 0.704 ms on config 3; as an LDS column: see HISTORY.md 3a).
    R* acc;
    __device__ inline V3<R> acc_get(int p) const { return mk<R>(acc[(p * 3) * DRT_BLOCK], acc[(p * 3 + 1) * DRT_BLOCK], acc[(p * 3 + 2) * DRT_BLOCK]); }
    __device__ inline void acc_set(int p, V3<R> v) { acc[(p * 3) * DRT_BLOCK] = v.x; acc[(p * 3 + 1) * DRT_BLOCK] = v.y; acc[(p * 3 + 2) * DRT_BLOCK] = v.z; }
    __device__ inline void new_path() { cnt[0] = 0; if (NC > 4) cnt[NC > 4 ? 1 : 0] = 0; zc = 0; }
};

// ---- ANY number of parameters (NP = DRT_NP_ANY) -------------------------------------------------------------------------
// The reference differentiates with respect to every Vector<T,3,true> of the scene, however many (vector.hpp:185-191;
// render.cpp:26-29 has four because its scene is small).  Counters and an LDS column per parameter (above) stop at eight.
// The general form keeps the same closed form -- dT/dc_p = T n_p / c_p, i.e. every vertex j that scattered on a colour adds
// g T E / (p_k c_{id_j}) to the row of ITS colour once the path meets a light -- and remembers WHICH colour every vertex
// scattered on instead of counting per colour:
//   history   8 bits per vertex (parameter ids < DRT_PATH_LDS_PARAMS = 136; 0xFF = no vertex): the last <= 4 in a register,
//             full words in an LDS column of the thread (dynamic shared memory: as many words as fit without costing the
//             kernel a block per CU -- four in the lockstep kernel: paths of 16 vertices; none in the regenerating ones),
//             deeper ones in a column of global memory (written once per four vertices, read where the path meets a light);
//   tables    per WAVE, in LDS: a row per channel of every parameter that requires a gradient (DevScene::grad_slot), in
//             2^clog2 copies (lane & (copies - 1): same-address atomics serialise), added to with ds_add -- one wave's adds
//             reach its own table in program order, so the sums do not depend on how the waves of the chip were scheduled;
//   per id    GenLds: the colour with zero channels replaced by 1 + its zero-count increments, 1 / c + row and zero-channel bits
//             (one ds_read_b128 each).
// A zero channel (red = (0.5, 0, 0), render.cpp:26): vertex j's own factor is the only zero of the channel iff zc_ch == 1, and
// then d/dc of that channel is T_ch (the product WITHOUT the zero factor, which is what the lane's T holds) -- else 0.
#define DRT_NP_ANY (-1)
// Blocks per CU (= waves per SIMD) the f32 lockstep k_path is compiled for, form by form (ms per launch on config 3's frame, the builds
// alternating in one process: profiles/r06_waves_per_simd.txt; five against six: r06_scratch_vs_waves.txt)
#ifndef DRT_LOCKSTEP_MIN_BLOCKS
#define DRT_LOCKSTEP_MIN_BLOCKS 7       // diffuse, <= 4 parameters: 72 registers.  Five (96 registers) 0.716, six (80) 0.695-0.702, seven 0.673, eight (64 + scratch) 0.694-0.702
#endif
#ifndef DRT_LOCKSTEP_GEN_MIN_BLOCKS
#define DRT_LOCKSTEP_GEN_MIN_BLOCKS 6   // its general form (any number of parameters): 77-80 registers; seven 0.725 -> 0.736
#endif
#ifndef DRT_LOCKSTEP_SPEC_MIN_BLOCKS
#define DRT_LOCKSTEP_SPEC_MIN_BLOCKS 6  // with the glossy lobe (config 5), <= 4 parameters: 78-80 registers; config 5's shape (2048 x 2048 x 16, depth 16): five 7.92, six 7.79,
                                        // seven 7.81 (tools/ab_kernel.py)
#endif
#ifndef DRT_LEAN_PATH_MIN_BLOCKS
#define DRT_LEAN_PATH_MIN_BLOCKS 8      // k_path_lean (no roulette in the loop, no emitting scatterer): 55 registers (forward only 49), no scratch, eight blocks' LDS in a CU (19,312 B each).
                                        // Seven (53 registers, 5.13e8 instructions against k_path's 5.36e8 -- and k_path's time) 0.640, eight 0.614, k_path 0.644;
                                        // through the kind-sorted program 0.830 / 0.795 / 0.904; forward only 0.621 / 0.623 / 0.629 (profiles/r15_path_lean.txt)
#endif
#ifndef DRT_REGEN_MIN_BLOCKS
#define DRT_REGEN_MIN_BLOCKS 5       // blocks per CU the f32 regenerating diffuse k_path is compiled for
#endif
#ifndef DRT_F64_MIN_BLOCKS
#define DRT_F64_MIN_BLOCKS 4         // blocks per CU the f64 lockstep diffuse k_path is compiled for: 128 registers instead of 142-145, four waves per
                                     // SIMD instead of three (config 3 in f64: 1.938 -> 1.890 ms, an albedo per shape 2.19 -> 1.97; 3 and 5: no gain)
#endif
// ... the forward-mode forms (NP = DRT_NP_TANGENT)
#ifndef DRT_TANGENT_MIN_BLOCKS
#define DRT_TANGENT_MIN_BLOCKS 6
#endif
#ifndef DRT_TANGENT_REGEN_MIN_BLOCKS
#define DRT_TANGENT_REGEN_MIN_BLOCKS 5
#endif
#ifndef DRT_TANGENT_F64_MIN_BLOCKS
#define DRT_TANGENT_F64_MIN_BLOCKS 3
#endif
// ... and their K-direction forms (NC = K: 9 K values per lane beside the forward-only kernel's, and 3 K sums in fp64; f64: twice that)
#ifndef DRT_TANGENTS2_MIN_BLOCKS
#define DRT_TANGENTS2_MIN_BLOCKS 5
#endif
#ifndef DRT_TANGENTS4_MIN_BLOCKS
#define DRT_TANGENTS4_MIN_BLOCKS 3
#endif
#ifndef DRT_TANGENTS8_MIN_BLOCKS
#define DRT_TANGENTS8_MIN_BLOCKS 2
#endif
#ifndef DRT_GEN_TABLE
#define DRT_GEN_TABLE 408            // elements of a wave's gradient table (rows x copies; 408 = 3 x DRT_PATH_LDS_PARAMS: one copy of every row at least)
#endif
template <bool B, typename X, typename Y> struct PickT { typedef X T; };
template <typename X, typename Y> struct PickT<false, X, Y> { typedef Y T; };
struct NoLds { int unused; };
template <bool B> struct BoolT { static constexpr bool value = B; };   // a compile-time tag for generic lambdas
// The tables are fp64 in the f32 kernels too (ds_add_f64): a table sums what 64 lanes x their samples add, and ONE heavy sample
// (the unbiased operator's L' g / pdf; a roulette-boosted path) in an f32 sum costs every later add its low bits -- measured
// with f32 tables: 3.4e-3 of the largest component on the 12-parameter unbiased fixture, where per-lane f32 sums give 3e-6.
template <typename R> struct GenAcc { typedef double T; };
#ifdef DRT_GEN_F32
template <> struct GenAcc<float> { typedef float T; };
#endif

template <typename R>
struct GenLds {
    R colnz[DRT_PATH_LDS_PARAMS][4];   // colour, zero channels replaced by 1 | [3]: zero-count increments, 8 bits per channel (pid_pack)
    R invc[DRT_PATH_LDS_PARAMS][4];    // 1 / c per channel, 0 where the channel is zero | [3]: table row | zero-channel bits << 16 (pid_pack)
    // The records of ONE parameter set (NP = DRT_NP_SETS_GRAD) live in tables sized by the scene's parameter count, not in a GenLds: this is
    // the view through which the general form's own code (add_emission's branch, add_word) reads that set's invc rows.  ONLY invc[id], id below
    // the scene's parameter count, may be read through it
    static __device__ inline const GenLds* over_invc(const R* rows) { return reinterpret_cast<const GenLds*>(rows - DRT_PATH_LDS_PARAMS * 4); }
};

template <typename R, typename SL>
__device__ inline void stage_gen(GenLds<R>& gl, const SL& lds, const DevScene<R>* __restrict__ sc)
{
    // (after stage_path_scene's barrier; ids beyond the scene's own read as (1, 1, 1) without a row)
    for (int p = threadIdx.x; p < DRT_PATH_LDS_PARAMS; p += blockDim.x) {
        const bool in = p < lds.sc.n_params;
        uint32_t zinc = 0, zbits = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const R c = in ? lds.params[p * 3 + ch] : R(1);
            const bool zero = zero_channel(c);
            gl.colnz[p][ch] = zero ? R(1) : c;
            gl.invc[p][ch] = zero ? R(0) : R(1) / c;
            zinc |= zero ? 1u << (8 * ch) : 0u;
            zbits |= zero ? 1u << ch : 0u;
        }
        const uint32_t slot = in ? (uint32_t)sc->grad_slot[p] : DRT_SLOT_NONE;
        gl.colnz[p][3] = pid_pack(R(0), zinc);
        gl.invc[p][3] = pid_pack(R(0), slot | zbits << 16);
    }
    __syncthreads();
}

template <typename R, int NC>
struct Tangents<R, DRT_NP_ANY, NC> {
    typedef typename GenAcc<R>::T GT;
    uint32_t cur;                   // the colours of the last <= 4 vertices, shifted in from the top (0xFF: none)
    uint32_t zc;                    // zero factors met per channel, 8 bits each
    uint32_t nv;                    // history entries of the current path (wave-uniform in the lockstep kernel)
    uint32_t* hist;                 // the thread's column of full history words: word w < hist_lds at hist[w * DRT_BLOCK] (LDS),
    uint32_t* hist_ovf;             // ... the others at hist_ovf[(w - hist_lds) * hist_stride] (global)
    uint32_t hist_lds, hist_stride;
    const GenLds<R>* gl;
    GT* table;                      // the wave's table, at the lane's copy: element (row, copy) at table[(row << clog2)]
    uint32_t clog2;
    R* acc;                         // (unused: the register / column forms' sums)
    // NC == 1, the gradient IMAGE (README.md:142-145; lockstep form, a lane IS a pixel): what the lane itself adds to the row of
    // the image's parameter, next to the wave's table
    V3<R> gsum;
    uint32_t gimg_row;
    __device__ inline void new_path() { cur = 0xFFFFFFFFu; zc = 0; nv = 0; }
    __device__ inline void store_word(uint32_t w, uint32_t v)
    {
        if (w < hist_lds) hist[w * DRT_BLOCK] = v;
        else hist_ovf[(size_t)(w - hist_lds) * hist_stride] = v;
    }
    __device__ inline uint32_t load_word(uint32_t w) const
    {
        return w < hist_lds ? hist[w * DRT_BLOCK] : hist_ovf[(size_t)(w - hist_lds) * hist_stride];
    }
    // one more vertex: `id` = the colour it scattered on, 0xFF = none (the path ended there).  UNIFORM: every lane of the wave
    // pushes at every bounce (the lockstep kernel: nv stays a scalar); else only lanes with `live`.
    template <bool UNIFORM>
    __device__ inline void push(bool live, uint32_t id)
    {
        const uint32_t shifted = (cur >> 8) | (id << 24);
        if (UNIFORM) {
            cur = shifted;
            ++nv;
            if ((nv & 3u) == 0u) {
                store_word((nv >> 2) - 1u, cur);
                cur = 0xFFFFFFFFu;
            }
        } else {
            cur = live ? shifted : cur;
            nv += live ? 1u : 0u;
            if (live && (nv & 3u) == 0u) {
                store_word((nv >> 2) - 1u, cur);
                cur = 0xFFFFFFFFu;
            }
        }
    }
    __device__ inline void add(uint32_t row, V3<R> v)
    {
        if constexpr (NC == 1) {
            const bool mine = row == gimg_row;
            gsum = mk<R>(gsum.x + (mine ? v.x : R(0)), gsum.y + (mine ? v.y : R(0)), gsum.z + (mine ? v.z : R(0)));
        }
        GT* t = table + ((row * 3u) << clog2);
        atomicAdd(t, (GT)v.x);
        atomicAdd(t + (1u << clog2), (GT)v.y);
        atomicAdd(t + (2u << clog2), (GT)v.z);
    }
    // the four vertices of one history word: each adds  TgE / c  (U where its own channel is the zero one) to its colour's row
    __device__ inline void add_word(uint32_t wd, V3<R> TgE, V3<R> U)
    {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t id = (wd >> (8 * b)) & 0xFFu;
            const bool valid = id != 0xFFu;
            if (wave_any(valid)) {
                if (valid) {
                    const R* rec = gl->invc[id];
                    const R ix = rec[0], iy = rec[1], iz = rec[2];
                    const uint32_t bits = pid_unpack(rec[3]);
                    const uint32_t row = bits & 0xFFFFu;
                    if (row != DRT_SLOT_NONE)
                        add(row, mk<R>((bits & 0x10000u) ? U.x : TgE.x * ix, (bits & 0x20000u) ? U.y : TgE.y * iy,
                                       (bits & 0x40000u) ? U.z : TgE.z * iz));
                }
            }
        }
    }
};

// ---- FORWARD mode: the derivative of the render along ONE direction of parameter space (NP = DRT_NP_TANGENT) -------------
// d radiance / d eps at params + eps v, per pixel (the reference's Dual<T>, dual.hpp, run through the path tracer): the product
// form above, contracted with v.  With T = prod_j c_{p_j} m_j,
//     dT_ch / d eps = T_ch sum_j v_{p_j,ch} / c_{p_j,ch}
// so a lane carries ONE running sum per channel, S_ch += v / c at every vertex its path goes on from -- for any number of
// parameters, without counters, vertex history or gradient tables.  Zero channels as above: T leaves the zero factors out and
// counts them (zc), and Z_ch sums v over the vertices whose channel is zero.  Where the path meets a light of emission e whose
// own tangent is e' (both / p_k):
//     zc_ch == 0:  T (e S + e')        zc_ch == 1:  T e Z   (the one zero factor's derivative is its v)        else 0
// Per parameter, in LDS (staged once per block from [params | v], which is what the kernel's `params` points at in this form):
// the colour with zero channels replaced by 1 + its zero-count increments, v / c (0 where the channel is zero), v where it is zero,
// and v itself for the lights.  Row DRT_PATH_LDS_PARAMS is the rest row of a lane whose path does not go on: colour (1, 1, 1), zeros.
#define DRT_NP_TANGENT (-2)
template <typename R>
struct DirLds {
    R colnz[DRT_PATH_LDS_PARAMS + 1][4];   // colour, zero channels replaced by 1 | [3]: zero-count increments, 8 bits per channel (pid_pack)
    R dlog[DRT_PATH_LDS_PARAMS + 1][4];    // v / c per channel, 0 where the channel is zero
    R dzero[DRT_PATH_LDS_PARAMS + 1][4];   // v where the channel is zero, else 0
    R dir[DRT_PATH_LDS_PARAMS * 3];        // v
};

template <typename R, typename SL>
__device__ inline void stage_dir(DirLds<R>& dl, const SL& lds, const R* __restrict__ params)
{
    // (after stage_path_scene's barrier; ids beyond the scene's own read as (1, 1, 1) with a zero direction)
    const int n = lds.sc.n_params < DRT_PATH_LDS_PARAMS ? lds.sc.n_params : DRT_PATH_LDS_PARAMS;
    for (int p = threadIdx.x; p <= DRT_PATH_LDS_PARAMS; p += blockDim.x) {
        const bool in = p < n;
        uint32_t zinc = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const R c = in ? lds.params[p * 3 + ch] : R(1);
            const R v = in ? params[(lds.sc.n_params + p) * 3 + ch] : R(0);
            const bool zero = zero_split(c, v, dl.colnz[p][ch], dl.dlog[p][ch], dl.dzero[p][ch]);
            zinc |= zero ? 1u << (8 * ch) : 0u;
            if (p < DRT_PATH_LDS_PARAMS)
                dl.dir[p * 3 + ch] = v;
        }
        dl.colnz[p][3] = pid_pack(R(0), zinc);
        dl.dlog[p][3] = R(0);
        dl.dzero[p][3] = R(0);
    }
    __syncthreads();
}

template <typename R>
struct Tangents<R, DRT_NP_TANGENT, 0> {
    uint32_t zc;                    // zero factors met per channel, 8 bits each
    V3<R> S, Z;                     // sums of v / c and of v (zero channels) over the vertices of the current path
    V3<R> dL;                       // d radiance / d eps of the current path
    const DirLds<R>* dl;
    R* acc;                         // (unused: the column form's sums)
    __device__ inline void new_path() { zc = 0; S = Z = dL = mk<R>(R(0), R(0), R(0)); }
};

// ---- ... along K directions in ONE render (NP = DRT_NP_TANGENT, NC = K in {2, 4, 8}; drt_hip_render_tangents) ----------------
// The path, its throughput T, the zero counts zc and the RNG key do not depend on the direction: K directions cost one path and K
// sets of (S, Z, dL).  The tables are sized by the SCENE's parameter count n, not by DRT_PATH_LDS_PARAMS (which would be ~6 KB per
// direction in f32): dynamic shared memory, in units of R, rows of four --
//     colnz[n + 1]                       the colour row, read once per bounce (row n: the rest row, colour (1, 1, 1), zeros)
//     dlog_k[n + 1], dzero_k[n + 1]      per direction k: v_k / c, and v_k where the channel is zero
//     dir_k[3 n]                         per direction: v_k itself, for the lights
// staged from [params | v_1 | ... | v_K] behind the kernel's `params`.  Every per-direction operation is the single-direction form's on
// that direction's own operands: direction k's sums do not see what the other directions hold, and a padded direction (all zeros) adds
// exact zeros.  Lockstep form only (a lane is a pixel): at the end of its sample range a lane writes its 3 K sums in the Jacobian form's
// layout, gpix[range][3 k + ch][pixel], for k below the caller's count (PathArgs::dirs_out()).
__host__ __device__ inline uint32_t dirs_table_words(uint32_t n, uint32_t K) { return (1u + 2u * K) * (n + 1u) * 4u + K * 3u * n; }
template <typename R, int K, typename SL>
__device__ inline void stage_dirs(R* __restrict__ tab, const SL& lds, const R* __restrict__ params)
{
    // (after stage_path_scene's barrier)
    const int n = lds.sc.n_params < DRT_PATH_LDS_PARAMS ? lds.sc.n_params : DRT_PATH_LDS_PARAMS;
    const int stride = (n + 1) * 4;
    R* dir = tab + (1 + 2 * K) * stride;
    for (int p = threadIdx.x; p <= n; p += blockDim.x) {
        const bool in = p < n;
        uint32_t zinc = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const R c = in ? lds.params[p * 3 + ch] : R(1);
            // (the rule alone, not zero_split(): the colour row is shared by the K directions and written once, and the split called per
            //  direction moved these kernels' instruction streams)
            const bool zero = zero_channel(c);
            tab[p * 4 + ch] = zero ? R(1) : c;
            zinc |= zero ? 1u << (8 * ch) : 0u;
            for (int k = 0; k < K; ++k) {
                const R v = in ? params[((size_t)(1 + k) * lds.sc.n_params + p) * 3 + ch] : R(0);
                tab[(1 + 2 * k) * stride + p * 4 + ch] = zero ? R(0) : v / c;
                tab[(2 + 2 * k) * stride + p * 4 + ch] = zero ? v : R(0);
                if (in)
                    dir[k * 3 * n + p * 3 + ch] = v;
            }
        }
        tab[p * 4 + 3] = pid_pack(R(0), zinc);
        for (int k = 0; k < K; ++k) {
            tab[(1 + 2 * k) * stride + p * 4 + 3] = R(0);
            tab[(2 + 2 * k) * stride + p * 4 + 3] = R(0);
        }
    }
    __syncthreads();
}

template <typename R, int NC>
struct Tangents<R, DRT_NP_TANGENT, NC> {
    uint32_t zc;                    // zero factors met per channel, 8 bits each (shared by the directions)
    V3<R> S[NC], Z[NC];             // per direction: sums of v / c and of v (zero channels) over the vertices of the current path
    V3<R> dL[NC];                   // ... d radiance / d eps of the current path
    const R* tab;                   // the block's tables (see above)
    uint32_t rest, stride;          // the rest row = the scene's parameter count; words of one table
    R* acc;                         // (unused: the column form's sums)
    __device__ inline void new_path()
    {
        zc = 0;
#pragma unroll
        for (int k = 0; k < NC; ++k)
            S[k] = Z[k] = dL[k] = mk<R>(R(0), R(0), R(0));
    }
};

// ---- ... with the samples' CROSS moments (NP = DRT_NP_CROSS, NC = K in {2, 4, 8}; drt_hip_render_normal_equations_cross) ------------
// The K-direction form above, unchanged in every operation on the path -- the same tables (stage_dirs), the same tangent_advance and
// tangent_emit on the same operands, so the radiance and derivative sums keep the bits drt_hip_render_tangents gives -- plus, per lane and
// after each sample, the raw moments an unbiased product of two pixel means needs (a U-statistic over the pixel's n samples):
//     Q_k[ch] += dL_k[ch] L[ch]          S2[ch] += L[ch]^2          in fp64, from the sample's own values (exact products for f32 operands)
// With T_k, m the pixel means and r = m - target:   mean over s != s' of t_{k,s} (L_s' - target) = T_k r - cov(t_k, L) / n, and of
// (L_s - target)(L_s' - target) = r^2 - var(L) / n, with the sample covariance (Q_k - n T_k m) / (n - 1) and variance (S2 - n m^2) / (n - 1).
// Raw moments add across sample ranges.  At the end of its range a lane writes gpix[range][row][pixel] with 6 nd + 3 rows: 3 nd derivative
// sums, 3 nd of Q, 3 of S2 (nd = PathArgs::dirs_out(), the caller's directions); k_cross_eq (below) forms the corrections per pixel.
#define DRT_NP_CROSS (-6)
#define DRT_NP_IS_DIR(np) ((np) == DRT_NP_TANGENT || (np) == DRT_NP_CROSS)
// blocks per CU (= waves per SIMD) of the f32 forms: the most that stay free of scratch (the compiler's report: DESIGN.md 9b)
#ifndef DRT_CROSS2_MIN_BLOCKS
#define DRT_CROSS2_MIN_BLOCKS 4
#endif
#ifndef DRT_CROSS4_MIN_BLOCKS
#define DRT_CROSS4_MIN_BLOCKS 3      // (diffuse; the glossy form with the reference's kinds compiled in keeps 8 bytes of scratch at three: two)
#endif
#ifndef DRT_CROSS8_MIN_BLOCKS
#define DRT_CROSS8_MIN_BLOCKS 2
#endif
template <typename R, int NC>
struct Tangents<R, DRT_NP_CROSS, NC> : Tangents<R, DRT_NP_TANGENT, NC> {
    double Q[NC][3], S2[3];         // the lane's moment sums over its sample range
};

// ---- ONE path under K parameter SETS (NP = DRT_NP_SETS, NC = K in {2, 4, 8}; drt_hip_render_param_sets) --------------------------
// A parameter is a colour or an emission and nothing else: the closest hit, the BxDF sample, the roulette and the draw indices do not
// see its value, so a path under parameter set A is the same path under set B.  K sets cost one ray, one key, one hit, one m_k and K
// pairs (T_k, L_k), moved by the forward-only form's own operations on set k's operands in its order:
//     per bounce  T_k = T_k * (col_k * m)          per light  L_k = L_k + T_k * (e_k * inv_pk)
// No zero-channel bookkeeping: a forward render keeps real zeros in T.  Tables: K of (n + 1) rows of four, n the SCENE's parameter
// count, in dynamic shared memory, staged from [params | P_1 | ... | P_K] behind the kernel's `params`; row n is the rest row (1, 1, 1)
// of a lane whose path does not go on.  Lockstep form only (a lane is a pixel): at the end of its sample range a lane writes its sums in
// the Jacobian form's layout, gpix[range][3 k + ch][pixel], for k below the caller's count (PathArgs::dirs_out()); the radiance partials
// (`fpart`, where the caller wants the plain image) are the sums of set K - 1, which the host fills with the context's own parameters.
#define DRT_NP_SETS (-3)
// blocks per CU (= waves per SIMD) of the f32 forms: the most that stay free of scratch (the compiler's report: DESIGN.md 9b)
#ifndef DRT_SETS2_MIN_BLOCKS
#define DRT_SETS2_MIN_BLOCKS 6
#endif
#ifndef DRT_SETS4_MIN_BLOCKS
#define DRT_SETS4_MIN_BLOCKS 4
#endif
#ifndef DRT_SETS8_MIN_BLOCKS
#define DRT_SETS8_MIN_BLOCKS 2
#endif
__host__ __device__ inline uint32_t sets_table_words(uint32_t n, uint32_t K) { return K * (n + 1u) * 4u; }
template <typename R, int K, typename SL>
__device__ inline void stage_sets(R* __restrict__ tab, const SL& lds, const R* __restrict__ params)
{
    // (after stage_path_scene's barrier)
    const int n = lds.sc.n_params < DRT_PATH_LDS_PARAMS ? lds.sc.n_params : DRT_PATH_LDS_PARAMS;
    for (int i = threadIdx.x; i < K * (n + 1); i += blockDim.x) {
        const int k = i / (n + 1), p = i - k * (n + 1);
        const R* src = params + ((size_t)(1 + k) * lds.sc.n_params + p) * 3;
        R* row = tab + (size_t)i * 4;
        row[0] = p < n ? src[0] : R(1);
        row[1] = p < n ? src[1] : R(1);
        row[2] = p < n ? src[2] : R(1);
        row[3] = R(0);
    }
    __syncthreads();
}

template <typename R, int NC>
struct Tangents<R, DRT_NP_SETS, NC> {
    V3<R> T[NC], L[NC];             // per set: prefix throughput and radiance of the current path
    const R* tab;                   // the block's tables (see above)
    uint32_t rest, stride;          // the rest row = the scene's parameter count; words of one table
    __device__ inline void new_path()
    {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            T[k] = mk<R>(R(1), R(1), R(1));
            L[k] = mk<R>(R(0), R(0), R(0));
        }
    }
};

// ---- ... each set with a DIRECTION of its own (NP = DRT_NP_SETS_ALONG, NC = K in {2, 4}; drt_hip_render_param_sets_along) ---------
// The product of the two forms above: one ray, one key, one hit, one m_k, and per set k the forward-mode form's state on set k's own
// operands -- the throughput T_k WITHOUT its zero factors, their counts zc_k (per set: the sets differ in which channels are zero), the sums
// S_k of d_k / c_k and Z_k of d_k over the zero channels, the radiance L_k (T_k masked by zc_k: a channel that met a zero is dark) and the
// derivative dL_k of the current path along d_k.  Every per-set operation is the single-direction form's (Tangents<R, DRT_NP_TANGENT, 0>) on
// that set's operands in its order: set k's sums see neither its companions nor the width.  Tables in dynamic shared memory, per set k and
// sized by the SCENE's parameter count n, in units of R --
//     colnz_k[n + 1], dlog_k[n + 1], dzero_k[n + 1]     rows of four: P_k with zero channels replaced by 1 | zero-count increments (pid_pack),
//                                                       d_k / P_k, and d_k where the channel is zero; row n: the rest row (1, 1, 1), zeros
//     par_k[3 n], dir_k[3 n]                            P_k and d_k themselves, for the lights (an emission is used as it is, zeros included)
// staged from [params | P_1 | d_1 | ... | P_K | d_K] behind the kernel's `params`.  Lockstep form only (a lane is a pixel): at the end of its
// sample range a lane writes 6 sums per set in the Jacobian form's layout, gpix[range][6 k + ch][pixel] (radiance) and
// gpix[range][6 k + 3 + ch][pixel] (derivative), for k below the caller's count (PathArgs::dirs_out()).
#define DRT_NP_SETS_ALONG (-4)
// blocks per CU (= waves per SIMD) of the f32 forms: the most that stay free of scratch (the compiler's report, DESIGN.md 9b: 121-128 registers
// at K = 2, 169-175 at K = 4; a block more spills 88 and 8 bytes per lane).  K = 8 was built and is not kept: 301 registers at one block per
// CU in f32, and its glossy f64 form spills at any budget
#ifndef DRT_SETS_ALONG2_MIN_BLOCKS
#define DRT_SETS_ALONG2_MIN_BLOCKS 4
#endif
#ifndef DRT_SETS_ALONG4_MIN_BLOCKS
#define DRT_SETS_ALONG4_MIN_BLOCKS 2
#endif
__host__ __device__ inline uint32_t sets_along_set_words(uint32_t n) { return 3u * (n + 1u) * 4u + 6u * n; }
__host__ __device__ inline uint32_t sets_along_table_words(uint32_t n, uint32_t K) { return K * sets_along_set_words(n); }
template <typename R, int K, typename SL>
__device__ inline void stage_sets_along(R* __restrict__ tab, const SL& lds, const R* __restrict__ params)
{
    // (after stage_path_scene's barrier)
    const int n = lds.sc.n_params < DRT_PATH_LDS_PARAMS ? lds.sc.n_params : DRT_PATH_LDS_PARAMS;
    const int stride = (n + 1) * 4, words = (int)sets_along_set_words((uint32_t)n);
    for (int i = threadIdx.x; i < K * (n + 1); i += blockDim.x) {
        const int k = i / (n + 1), p = i - k * (n + 1);
        const bool in = p < n;
        const R* P = params + ((size_t)(1 + 2 * k) * lds.sc.n_params + p) * 3;
        const R* D = params + ((size_t)(2 + 2 * k) * lds.sc.n_params + p) * 3;
        R* set = tab + (size_t)k * words;
        uint32_t zinc = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const R c = in ? P[ch] : R(1);
            const R v = in ? D[ch] : R(0);
            const bool zero = zero_split(c, v, set[p * 4 + ch], set[stride + p * 4 + ch], set[2 * stride + p * 4 + ch]);
            zinc |= zero ? 1u << (8 * ch) : 0u;
            if (in) {
                set[3 * stride + p * 3 + ch] = c;
                set[3 * stride + 3 * n + p * 3 + ch] = v;
            }
        }
        set[p * 4 + 3] = pid_pack(R(0), zinc);
        set[stride + p * 4 + 3] = R(0);
        set[2 * stride + p * 4 + 3] = R(0);
    }
    __syncthreads();
}

template <typename R, int NC>
struct Tangents<R, DRT_NP_SETS_ALONG, NC> {
    V3<R> T[NC], L[NC];             // per set: prefix throughput (zero factors left out) and radiance of the current path
    V3<R> S[NC], Z[NC], dL[NC];     // ... sums of d / c and of d (zero channels) over its vertices, its derivative along the set's direction
    uint32_t zc[NC];                // ... zero factors met per channel, 8 bits each
    const R* tab;                   // the block's tables (see above)
    uint32_t rest, stride, words;   // the rest row = the scene's parameter count; words of one table of rows, of one set
    __device__ inline void new_path()
    {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            T[k] = mk<R>(R(1), R(1), R(1));
            L[k] = S[k] = Z[k] = dL[k] = mk<R>(R(0), R(0), R(0));
            zc[k] = 0;
        }
    }
};

// ---- REVERSE mode under K parameter sets: every set's summed gradient J(P_k)^T w_k in one trace (NP = DRT_NP_SETS_GRAD, NC = K in {2, 4, 8};
// drt_hip_render_param_sets_grad) ----
// The general gradient form (Tangents<R, DRT_NP_ANY>) remembers WHICH colour every vertex scattered on, and that history does not see a
// parameter's value either: K sets share the ray, the key, the hit, m_k AND the history (`h`: cur, nv, the LDS words, the global overflow
// column).  Per set k a lane keeps the throughput T_k without its zero factors, their counts zc_k (the sets differ in which channels are
// zero) and the pixel's seed g_k (read once per pixel from adjoint + k W H 3): seven registers.  Where the path meets a light -- mid-path on
// a shape with BxDF and emitter, or at its end -- set k runs add_emission's general branch AS IT IS on its own operands: `h` is pointed at
// the set's zero counts, its invc rows (GenLds::over_invc), its raw parameters (SetParams: an emission is used as it is, zeros included) and
// its rows of the wave's table, k R + slot with R = 3 rows per parameter that requires a gradient.  The table keeps its DRT_GEN_TABLE elements
// for K R rows in the largest power-of-two number of copies that fits; K is the instantiated width, so a set's sums do not depend on how
// many of the K the caller gave.  Padded sets (k at and above the caller's count, which rides in PathArgs::gimg_row) add nothing.  Tables in
// dynamic shared memory BEHIND the history words (PathArgs::hist_lds of them per thread), per set k and sized by the SCENE's parameter count n,
// in units of R --
//     colnz_k[n + 1], invc_k[n + 1]      rows of four, as GenLds keeps them: P_k with zero channels replaced by 1 | zero-count increments, and
//                                        1 / P_k | table row, zero-channel bits; row n of colnz: the rest row (1, 1, 1), zeros
//     par_k[3 n] (padded to rows of four)  P_k itself, for the lights
// staged from [params | P_1 | ... | P_K] behind the kernel's `params`.  Lockstep form only.  PathArgs::gen_rows counts ALL K R rows: the
// block's row sums leave through gen_finish as the general form's do, and k_sets_grad_finish maps them back to out[k][parameter][channel].
#define DRT_NP_SETS_GRAD (-5)
// blocks per CU (= waves per SIMD) of the f32 forms: the most at which every instantiation stays free of scratch AND the static LDS plus the
// largest tables (136 parameters) fit the CU (the compiler's report: DESIGN.md 9b).  The compiler takes 74-83 registers at K = 2, 103-105 at
// K = 4 and 163-165 at K = 8 whatever the bound: the registers would allow 6-5, 4 and 3 blocks, the tables at 136 parameters 4, 3 and 2
#ifndef DRT_SETS_GRAD2_MIN_BLOCKS
#define DRT_SETS_GRAD2_MIN_BLOCKS 4
#endif
#ifndef DRT_SETS_GRAD4_MIN_BLOCKS
#define DRT_SETS_GRAD4_MIN_BLOCKS 3
#endif
#ifndef DRT_SETS_GRAD8_MIN_BLOCKS
#define DRT_SETS_GRAD8_MIN_BLOCKS 2
#endif
__host__ __device__ inline uint32_t sets_grad_set_words(uint32_t n) { return 2u * (n + 1u) * 4u + ((3u * n + 3u) & ~3u); }
__host__ __device__ inline uint32_t sets_grad_table_words(uint32_t n, uint32_t K) { return K * sets_grad_set_words(n); }
template <typename R, int K, typename SL>
__device__ inline void stage_sets_grad(R* __restrict__ tab, const SL& lds, const DevScene<R>* __restrict__ sc, const R* __restrict__ params)
{
    // (after stage_path_scene's barrier; the records are stage_gen's, of set k's values)
    const int n = lds.sc.n_params < DRT_PATH_LDS_PARAMS ? lds.sc.n_params : DRT_PATH_LDS_PARAMS;
    const int stride = (n + 1) * 4, words = (int)sets_grad_set_words((uint32_t)n);
    for (int i = threadIdx.x; i < K * (n + 1); i += blockDim.x) {
        const int k = i / (n + 1), p = i - k * (n + 1);
        const bool in = p < n;
        const R* P = params + ((size_t)(1 + k) * lds.sc.n_params + p) * 3;
        R* set = tab + (size_t)k * words;
        uint32_t zinc = 0, zbits = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const R c = in ? P[ch] : R(1);
            const bool zero = zero_channel(c);
            set[p * 4 + ch] = zero ? R(1) : c;
            set[stride + p * 4 + ch] = zero ? R(0) : R(1) / c;
            zinc |= zero ? 1u << (8 * ch) : 0u;
            zbits |= zero ? 1u << ch : 0u;
            if (in)
                set[2 * stride + p * 3 + ch] = c;
        }
        const uint32_t slot = in ? (uint32_t)sc->grad_slot[p] : DRT_SLOT_NONE;
        set[p * 4 + 3] = pid_pack(R(0), zinc);
        set[stride + p * 4 + 3] = pid_pack(R(0), slot | zbits << 16);
    }
    __syncthreads();
}

template <typename R, int NC>
struct Tangents<R, DRT_NP_SETS_GRAD, NC> {
    typedef typename GenAcc<R>::T GT;
    V3<R> T[NC], g[NC];             // per set: prefix throughput (zero factors left out); the pixel's seed
    uint32_t zc[NC];                // ... zero factors met per channel, 8 bits each
    Tangents<R, DRT_NP_ANY, 0> h;   // shared by the sets: the path's history; and the general form's view of ONE set, pointed at set k for its turn
    const R* tab;                   // the block's tables (see above)
    uint32_t rest, stride, words;   // the rest row = the scene's parameter count; words of one table of rows, of one set
    GT* table;                      // the wave's table, at the lane's copy (set 0's first row)
    uint32_t set_rows, n_sets;      // R: table rows of one set; the caller's sets
    __device__ inline void new_path()
    {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            T[k] = mk<R>(R(1), R(1), R(1));
            zc[k] = 0;
        }
        h.new_path();
    }
    // the general form's view, at set k
    __device__ inline void point_at(int k)
    {
        const R* set = tab + (uint32_t)k * words;
        h.zc = zc[k];
        h.gl = GenLds<R>::over_invc(set + stride);
        h.table = table + (((uint32_t)k * set_rows) << h.clog2);
    }
    __device__ inline SetParams<R> params_of(int k) const { return SetParams<R>{tab + (uint32_t)k * words + 2u * stride}; }
};

// ---- the forward-mode step, once: what the single-direction form, every direction of the K-direction form and every set of the sets-along
// form do to their own operands (so a direction's or a set's sums equal the single-direction form's bit for bit: one function, not three
// copies).  Operand-level: none of them knows which form calls it.
// ... per bounce, from the rows of v / c and of v (zero channels) of the colour the path scattered on
template <typename R>
__device__ inline void tangent_advance(const R* ds, const R* dz, V3<R>& S, V3<R>& Z)
{
    S = mk<R>(S.x + ds[0], S.y + ds[1], S.z + ds[2]);
    Z = mk<R>(Z.x + dz[0], Z.y + dz[1], Z.z + dz[2]);
}
// ... at a light of emission E (already / p_k) whose tangent is vd: dL += T (E S + vd / p_k) where no factor of the channel is zero,
// T E Z where exactly one is (T leaves the zero factors out), else nothing
template <typename R>
__device__ inline void tangent_emit(V3<R> T, uint32_t zc, V3<R> E, const R* vd, R inv_pk, V3<R> S, V3<R> Z, V3<R>& dL)
{
    const V3<R> Ed = mk<R>(vd[0], vd[1], vd[2]) * inv_pk;
    const V3<R> d0 = mk<R>(fma_r(E.x, S.x, Ed.x), fma_r(E.y, S.y, Ed.y), fma_r(E.z, S.z, Ed.z));
    const V3<R> d1 = E * Z;
    const uint32_t zx = zc & 0xFFu, zy = zc & 0xFF00u, zz = zc & 0xFF0000u;
    dL = mk<R>(fma_r(T.x, zx == 0u ? d0.x : (zx == 0x1u ? d1.x : R(0)), dL.x),
               fma_r(T.y, zy == 0u ? d0.y : (zy == 0x100u ? d1.y : R(0)), dL.y),
               fma_r(T.z, zz == 0u ? d0.z : (zz == 0x10000u ? d1.z : R(0)), dL.z));
}

// ---- the three forms whose tables live in dynamic shared memory (K directions, K sets, K sets with a direction each): the form's
// staging, then the thread's view of the block's tables (after stage_path_scene's barrier)
template <typename R, int NP, int NC, typename SL>
__device__ inline void path_tables_begin(Tangents<R, NP, NC>& tg, const SL& lds, const R* __restrict__ params)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dirs[];
    R* tab = reinterpret_cast<R*>(s_dirs);
    if constexpr (NP == DRT_NP_SETS_ALONG)
        stage_sets_along<R, NC>(tab, lds, params);
    else if constexpr (NP == DRT_NP_SETS)
        stage_sets<R, NC>(tab, lds, params);
    else
        stage_dirs<R, NC>(tab, lds, params);
    tg.tab = tab;
    tg.rest = (uint32_t)(lds.sc.n_params < DRT_PATH_LDS_PARAMS ? lds.sc.n_params : DRT_PATH_LDS_PARAMS);
    tg.stride = (tg.rest + 1u) * 4u;
    if constexpr (NP == DRT_NP_SETS_ALONG)
        tg.words = sets_along_set_words(tg.rest);
    tg.new_path();
}

// what a block of a general-form kernel keeps in LDS, and the two ends of its life
template <typename R>
struct GenBlock {
    GenLds<R> gl;
    typename GenAcc<R>::T table[DRT_BLOCK / DRT_WAVE][DRT_GEN_TABLE];
};
// (before stage_path_scene's barrier: the tables start at zero)
template <typename R>
__device__ inline void gen_zero(GenBlock<R>& gb)
{
    typedef typename GenAcc<R>::T GT;
    for (uint32_t i = threadIdx.x; i < (DRT_BLOCK / DRT_WAVE) * DRT_GEN_TABLE; i += DRT_BLOCK)
        (&gb.table[0][0])[i] = GT(0);
}
// (after it: the per-id records; the thread's view of its wave's table)
template <typename R, int NC, typename SL>
__device__ inline void gen_begin(GenBlock<R>& gb, const SL& lds, const DevScene<R>* __restrict__ sc, const PathArgs& a, uint32_t* hist,
                                 uint32_t* hist_ovf, Tangents<R, DRT_NP_ANY, NC>& tg)
{
    stage_gen(gb.gl, lds, sc);
    tg.gl = &gb.gl;
    tg.hist = hist + threadIdx.x;
    tg.hist_ovf = hist_ovf + (size_t)blockIdx.x * DRT_BLOCK + threadIdx.x;
    tg.gsum = mk<R>(R(0), R(0), R(0));
    tg.gimg_row = a.gimg_row;
    tg.hist_lds = a.hist_lds;
    tg.hist_stride = a.hist_stride;
    tg.clog2 = a.gen_clog2;
    tg.table = &gb.table[threadIdx.x / DRT_WAVE][threadIdx.x & ((1u << a.gen_clog2) - 1u)];
    tg.acc = nullptr;
    tg.new_path();
}
// the waves' tables -> the block's row sums in fp64: copies, then waves, in a fixed order; K7 / the finishing launch adds the blocks
template <typename R>
__device__ inline void gen_finish(const GenBlock<R>& gb, const PathArgs& a, double* __restrict__ gpart)
{
    __syncthreads();
    const uint32_t copies = 1u << a.gen_clog2;
    for (uint32_t r = threadIdx.x; r < a.gen_rows; r += DRT_BLOCK) {
        double v = 0;
        for (int ww = 0; ww < DRT_BLOCK / DRT_WAVE; ++ww)
            for (uint32_t c = 0; c < copies; ++c)
                v += (double)gb.table[ww][(r << a.gen_clog2) + c];
        gpart[(size_t)blockIdx.x * a.gen_rows + r] = v;
    }
}

// NP = DRT_NP_SETS_GRAD: the general form's block -- its zeroed tables, the shared history (gen_begin, on `h`) -- and the K sets' own tables in
// dynamic shared memory behind the history words (after stage_path_scene's barrier)
template <typename R, int NC, typename SL>
__device__ inline void sets_grad_begin(GenBlock<R>& gb, const SL& lds, const DevScene<R>* __restrict__ sc, const R* __restrict__ params, const PathArgs& a,
                                       Tangents<R, DRT_NP_SETS_GRAD, NC>& tg)
{
    // (the launch's one dynamic block: [hist_lds][DRT_BLOCK] history words, then the tables -- declared as path_tables_begin declares it, for its alignment)
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dirs[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(s_dirs);
    gen_begin(gb, lds, sc, a, hist, reinterpret_cast<uint32_t*>(a.hist_ovf), tg.h);
    R* tab = reinterpret_cast<R*>(hist + (size_t)a.hist_lds * DRT_BLOCK);
    stage_sets_grad<R, NC>(tab, lds, sc, params);
    tg.tab = tab;
    tg.rest = (uint32_t)(lds.sc.n_params < DRT_PATH_LDS_PARAMS ? lds.sc.n_params : DRT_PATH_LDS_PARAMS);
    tg.stride = (tg.rest + 1u) * 4u;
    tg.words = sets_grad_set_words(tg.rest);
    tg.table = tg.h.table;
    tg.set_rows = a.gen_rows / (uint32_t)NC;
    tg.n_sets = a.gimg_row < (uint32_t)NC ? a.gimg_row : (uint32_t)NC;
#pragma unroll
    for (int k = 0; k < NC; ++k)
        tg.g[k] = mk<R>(R(1), R(1), R(1));
    tg.new_path();
}

// ---- the roles of the fast path's parameter slots ------------------------------------------------------------------------
// The reference's scene has three albedos that never emit and one emission that never scatters (render.cpp:26-29); a scene of the
// ABI may use any parameter as both.  What the scene's records say about it (drt_hip_upload_scene: every material's colour parameter,
// every emitter's parameter) reaches the lockstep k_path as part of its NC template argument,
//     nc | colour mask << 8 | emission mask << 16        (bit p of a mask: slot p can have that role; DRT_NC_ROLES)
// so a kernel's name says what it was compiled for and the library's instantiations and hiprtc's are the same source.  Masks of zero
// mean "not known": every slot below NC may be a colour, every slot an emission -- the code every other form keeps.
#define DRT_NC_ROLES(nc, colour_mask, emission_mask) ((int)(nc) | (int)(colour_mask) << 8 | (int)(emission_mask) << 16)
#define DRT_NC_OF(ncr) ((int)(ncr) & 0x3F)
#define DRT_ROLES_OF(ncr) ((int)(ncr) >> 8)
// ... and in the low byte, above the column count, one bit: the JACOBIAN form of the lockstep column kernels (drt_hip_render_normal_equations) -- at the end of its
// sample range a lane writes EVERY row of its gradient column out per pixel (the gradient image writes one), and the block's sums are not formed
#define DRT_NC_JACOBIAN 0x40
#define DRT_JACOBIAN_OF(ncr) ((((int)(ncr)) & DRT_NC_JACOBIAN) != 0)
#define DRT_ROLES_CORNELL DRT_ROLES_OF(DRT_NC_ROLES(0, 0x7, 0x8))      // render.cpp:26-29: colour, colour, colour, emission
template <int NP, int NC, int ROLES>
struct PathRoles {
    static constexpr int all = NP > 0 ? (1 << NP) - 1 : 0;
    static constexpr int colm = ROLES ? (ROLES & 0xFF) & ((1 << NC) - 1) : (1 << NC) - 1;
    static constexpr int emitm = ROLES ? (ROLES >> 8) & all : all;
    static __device__ constexpr bool colour(int p) { return (colm >> p) & 1; }
    static __device__ constexpr bool emission(int p) { return (emitm >> p) & 1; }
    static __device__ constexpr bool only_emission(int p) { return emitm == (1 << p); }
};

// an emissive vertex reached with prefix throughput T: radiance and gradients
//   L     += T E / p_k                                   (pathtracer.hpp:113-114, 133)
//   d/dc_p += g dT_p E / p_k      d/dE += g T / p_k       (vector.hpp:418-484 in closed form)
// LOSS (DRT_RENDER_LOSS_L2, the end of a path only): `g` holds the lane's TARGET pixel and the seed is the derivative of the
// sample's own squared error, 2 (L - target), with L the path's radiance INCLUDING this emission -- final where the path ends
// on a light without BxDF, which is the only emissive vertex of a path in the scenes this form is used for.
// ROLES (PathRoles, below; 0 = every slot may be both): which of the NP slots can be a BxDF's colour and which can be a light's
// emission, as compile-time facts.  A slot that is no emission loses the one-hot term `own ? gT : 0` (+ 0 changes no bit of a sum that
// is never -0), the only emission slot of a scene takes gT without asking, a slot that is no colour loses its counter, its 1 / c row and
// its zero-channel cases, a slot that is neither is not touched.  Every term that remains is the same operation on the same operands
// in the same order: the sums keep their bits.
template <typename R, int NP, int NC, bool LOSS = false, typename SL = PathSceneLds<R>, int ROLES = 0>
__device__ inline void add_emission(const SL& lds, const TangentLds<R>& tl, const R* __restrict__ params, uint32_t eid, R inv_pk,
                                    V3<R> T, V3<R> g, V3<R>& L, Tangents<R, NP, NC>& tg
#ifdef DRT_SAMPLE_LOSS
                                    , const R* loss_q = nullptr
#endif
                                    )
{
    if constexpr (NP == DRT_NP_SETS) {
        // K parameter sets: the forward-only form's L = L + T (e inv_pk), once per set on the set's own emission, T and L
        const R* er = tg.tab + (eid < tg.rest ? eid : 0u) * 4u;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const R* e = er + (uint32_t)k * tg.stride;
            const V3<R> Ek = mk<R>(e[0], e[1], e[2]) * inv_pk;
            tg.L[k] = tg.L[k] + tg.T[k] * Ek;
        }
    } else if constexpr (NP == DRT_NP_SETS_ALONG) {
        // K sets, a direction each: the single-direction forward case below (tangent_emit), once per set on the set's own emission, its tangent,
        // T, zc, S, Z.  (The radiance add's dark channels share their three masks with the tangent add: written here, not taken from a function
        // shared with the general branch below -- that moved these kernels' instruction streams)
        const uint32_t er = 3u * tg.stride + (eid < tg.rest ? eid : 0u) * 3u;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const R* e = tg.tab + (uint32_t)k * tg.words + er;
            const R* vd = e + 3u * tg.rest;
            const V3<R> Tk = tg.T[k];
            const V3<R> Ek = mk<R>(e[0], e[1], e[2]) * inv_pk;
            const uint32_t zx = tg.zc[k] & 0xFFu, zy = tg.zc[k] & 0xFF00u, zz = tg.zc[k] & 0xFF0000u;
            const V3<R> Tr = mk<R>(zx ? R(0) : Tk.x, zy ? R(0) : Tk.y, zz ? R(0) : Tk.z);
            tg.L[k] = tg.L[k] + Tr * Ek;
            tangent_emit(Tk, tg.zc[k], Ek, vd, inv_pk, tg.S[k], tg.Z[k], tg.dL[k]);
        }
    } else if constexpr (NP == DRT_NP_SETS_GRAD) {
        // K sets, a gradient each: the general branch below, once per set the caller gave, on the set's own emission, T, zc, seed, invc rows and
        // table rows (the radiance it also forms is not kept: this form has no image)
#pragma unroll
        for (int k = 0; k < NC; ++k)
            if ((uint32_t)k < tg.n_sets) {
                tg.point_at(k);
                V3<R> Lk = mk<R>(R(0), R(0), R(0));
                add_emission<R, DRT_NP_ANY, 0, false, SetParams<R>>(tg.params_of(k), tl, params, eid, inv_pk, tg.T[k], tg.g[k], Lk, tg.h);
            }
    } else {
        const V3<R> E = load_param<R, (NP != 0)>(lds, params, (int)eid) * inv_pk;
        V3<R> Tr = T;
        if (NC > 0 || NP == DRT_NP_ANY || DRT_NP_IS_DIR(NP))  // a channel that met a zero colour is dark
            Tr = mk<R>((tg.zc & 0xFFu) ? R(0) : T.x, (tg.zc & 0xFF00u) ? R(0) : T.y, (tg.zc & 0xFF0000u) ? R(0) : T.z);
        L = L + Tr * E;
        if constexpr (DRT_NP_IS_DIR(NP) && NC > 0) {
            // K directions: the single-direction case below (tangent_emit), once per direction
            const R* dir = tg.tab + (1u + 2u * NC) * tg.stride + (eid < tg.rest ? eid : 0u) * 3u;
#pragma unroll
            for (int k = 0; k < NC; ++k)
                tangent_emit(T, tg.zc, E, dir + (uint32_t)k * 3u * tg.rest, inv_pk, tg.S[k], tg.Z[k], tg.dL[k]);
        } else
        if constexpr (NP == DRT_NP_TANGENT) {
            // forward mode: T (e S + e') where no factor of the channel is zero, T e Z where exactly one is
            tangent_emit(T, tg.zc, E, tg.dl->dir + (eid < DRT_PATH_LDS_PARAMS ? eid : 0u) * 3u, inv_pk, tg.S, tg.Z, tg.dL);
        } else
        if constexpr (NP == DRT_NP_ANY) {
            // any number of parameters: the light's own row, then every vertex of the path's history adds to its colour's row
#ifdef DRT_SAMPLE_LOSS
            if (LOSS) {
                R value_;
                V3<R> seed_ = mk<R>(R(0), R(0), R(0));
                sample_loss<R>(loss_q, L, g, value_, seed_);
                g = seed_;
            }
#else
            if (LOSS)
                g = mk<R>(R(2) * (L.x - g.x), R(2) * (L.y - g.y), R(2) * (L.z - g.z));
#endif
            const V3<R> gE = g * E;
            const uint32_t ebits = pid_unpack(tg.gl->invc[eid < DRT_PATH_LDS_PARAMS ? eid : 0][3]);
            if ((ebits & 0xFFFFu) != DRT_SLOT_NONE && eid < DRT_PATH_LDS_PARAMS)
                tg.add(ebits & 0xFFFFu, g * Tr * inv_pk);
            const V3<R> TgE = Tr * gE;
            const V3<R> U = mk<R>((tg.zc & 0xFFu) == 0x1u ? T.x * gE.x : R(0), (tg.zc & 0xFF00u) == 0x100u ? T.y * gE.y : R(0),
                                  (tg.zc & 0xFF0000u) == 0x10000u ? T.z * gE.z : R(0));
            const uint32_t nw = tg.nv >> 2;
            for (uint32_t w = 0; wave_any(w < nw); ++w)
                tg.add_word(w < nw ? tg.load_word(w) : 0xFFFFFFFFu, TgE, U);
            tg.add_word(tg.cur, TgE, U);
        } else
        if constexpr (NP > 0) {
            if (NC > 0)
                asm volatile("" ::: "memory");    // (keeps the reads of `tl` below where they are: see there)
#ifdef DRT_SAMPLE_LOSS
            if (LOSS) {
                R value_;
                V3<R> seed_ = mk<R>(R(0), R(0), R(0));
                sample_loss<R>(loss_q, L, g, value_, seed_);
                g = seed_;
            }
#else
            if (LOSS)
                g = mk<R>(R(2) * (L.x - g.x), R(2) * (L.y - g.y), R(2) * (L.z - g.z));
#endif
            const V3<R> gE = g * E, gT = g * Tr * inv_pk;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                typedef PathRoles<NP, NC, ROLES> RL;
                const bool is_colour = (RL::colm >> p) & 1, is_emission = (RL::emitm >> p) & 1;
                if (ROLES != 0 && !is_colour && !is_emission)
                    continue;
                const bool own = (ROLES != 0 && RL::emitm == (1 << p)) || eid == (uint32_t)p;
                const V3<R> ap = tg.acc_get(p);
                V3<R> a0 = mk<R>(ap.x + (own ? gT.x : R(0)), ap.y + (own ? gT.y : R(0)), ap.z + (own ? gT.z : R(0)));
                if (ROLES != 0 && !is_emission)
                    a0 = ap;
                if (is_colour) {
                    const uint32_t n = (tg.cnt[p >> 2] >> (8 * (p & 3))) & 0xFFu;
                    const R nf = (R)(int)n;
                    // (read where they are used, once per sample: hoisted out of the sample loop these twelve wave-uniform words
                    //  cost the kernel its fifth wave per SIMD)
                    V3<R> dT = mk<R>(Tr.x * (nf * tl.invc[p][0]), Tr.y * (nf * tl.invc[p][1]), Tr.z * (nf * tl.invc[p][2]));
                    const uint32_t zb = __builtin_amdgcn_readfirstlane(tl.inc[p][3]);
                    if (zb) {
                        const bool one = n == 1u;
                        if (zb & 1u) dT.x = (one && (tg.zc & 0xFFu) == 0x1u) ? T.x : R(0);
                        if (zb & 2u) dT.y = (one && (tg.zc & 0xFF00u) == 0x100u) ? T.y : R(0);
                        if (zb & 4u) dT.z = (one && (tg.zc & 0xFF0000u) == 0x10000u) ? T.z : R(0);
                    }
                    tg.acc_set(p, mk<R>(fma_r(dT.x, gE.x, a0.x), fma_r(dT.y, gE.y, a0.y), fma_r(dT.z, gE.z, a0.z)));
                } else
                    tg.acc_set(p, a0);
            }
        }
    }
}

template <typename R>
struct CameraLane {            // per-lane camera constants (the lane's pixel does not change over its samples)
    R cs0, ct0;                // (2 x / W - 1) aspect tan(vfov / 2) and (2 y / H - 1) tan(vfov / 2) at the pixel's corner
};

// ---- one bounce of one path (every lane executes it; `live` says whether the lane's path is still going) -----------
// pk, inv_pk, n_theta, next_rr, next_cap describe the depth of the vertex: wave-uniform scalars in the fixed-depth
// kernel (all lanes at the same depth), per-lane values in the regenerating one.  On return: ra/rb = the next ray,
// T/dT moved on iff `alive`; `on_light` = the path ended on a light without BxDF (pathtracer.hpp:38-39: f = 0) whose
// emission parameter is `light` -- the caller adds that emission (the fixed-depth kernel once per sample, after its
// bounce loop, for all lanes together; the regenerating kernel when the lane's path ends).
// what the unbiased backward needs to know about a vertex (it re-samples a fresh direction there)
template <typename R>
struct PathVertex {
    V3<R> P, nrm, d;           // point, normal, direction of the ray that arrived
    uint32_t ids;              // colour | emission << 16 parameter ids
    int material;              // index of the BxDF's material record (valid when scattered)
    bool hit, scattered;       // the ray hit something / something with a BxDF
};

// FIXED, NO_LIT_BXDF (k_path_lean, below; no other caller names them): what the host knows about the render and the scene as
// compile-time facts -- no vertex inside the loop sees the roulette and the cap IS the roulette's, so no draw, no capped path; no shape
// that scatters also emits, so no emission is added here.
// LIGHTS (k_path_lean again) != 0: the scene's pure lights (an emitter, no BxDF) as a bit set in scene order -- at the `last` vertex, where
// only on_light and light leave the bounce, the hit is light_end_sig (drt_prog.h): the closest light and whether anything hides it, no
// closest hit over all shapes, no read of the hit's record.
template <typename R, bool SPEC, int NP, int NC, typename SG, bool FREEZE_BY_ROW = false, bool FIXED = false, bool NO_LIT_BXDF = false,
          unsigned long long LIGHTS = 0ull>
__device__ inline void path_bounce(const PathArgs& a, const PathSceneLds<R>& lds, const TangentLds<R>& tl, const DevScene<R>* __restrict__ sc,
                                   const R* __restrict__ params, const ProgRecs<SG::n, R>& recs, uint32_t key,
                                   R pk, R inv_pk, uint32_t n_theta, bool next_rr, bool next_cap, bool live, V3<R> g,
                                   typename Q4<R>::T& ra, typename Q2<R>::T& rb, V3<R>& T, V3<R>& L, Tangents<R, NP, NC>& tg,
                                   bool& alive, bool& capped, bool& on_light, uint32_t& light, PathVertex<R>* vo = nullptr,
                                   bool last = false, const float* __restrict__ seed_px = nullptr, const uint32_t* ih = nullptr,
                                   const LeanLds<SG::n, NC>* ll = nullptr, uint64_t* live_mask = nullptr, uint32_t kf = 0u, uint32_t* end_ids = nullptr)
{
    static_assert(LIGHTS == 0ull || (sizeof(R) == 4 && SG::n > 0 && FIXED && NO_LIT_BXDF), "LIGHTS: k_path_lean's compiled-in program");
    // FOLDED (k_path_lean beside a compiled-in program): `kf` is the sample's folded key (path_camera) and a draw is combine_folded
    // (drt_fold.h) of it and the folded h(n) -- the scalar unit's, as h(n) is: one exclusive-or a lane where the plain draw has two
    constexpr bool FOLDED = DRT_LEAN_FOLD_DRAWS != 0 && FIXED && SG::n > 0;
    // LEAN_REC (k_path_lean's facts beside a compiled-in program): the hit's record and the colour's row come from `ll` (LeanLds)
    constexpr bool LEAN_REC = lean_rec<SG, NC, FREEZE_BY_ROW, FIXED, NO_LIT_BXDF, SPEC, R>();
    // (ih, the forms whose lanes stand at their own depths: the draw indices' hash rounds h(n) as a table in LDS -- where all
    //  lanes of a wave share the index, the lockstep kernel, the scalar unit computes h(n) and the table would only cost)
    auto draw = [&](uint32_t n) {
        if constexpr (FOLDED)
            return combine_folded(fold16(drt_rng_index_hash(a.rng_stream, n)), kf);
        else
            return ih ? drt_rng_combine(ih[n], key) : rng_draw(a.rng_stream, key, n);
    };
    // (seed_px, the regenerating form: where the pixel's adjoint seed stands in the caller's image -- read only where a vertex
    //  emits, instead of carrying it in registers for a lane that changes pixel with every path)
    // `last` (wave-uniform; the lockstep kernel at the deepest vertex a path can have): no lane's path goes on from here, so
    // nothing is sampled -- the reference does sample a direction there, and the trace() it hands it to is absorbed before it
    // casts a ray (pathtracer.hpp:128): a factor of exactly 0.  What is left of the bounce is the hit, the light it may have
    // ended on, and the count of paths a user cap (not the roulette) cut short.  Same results bit for bit, ~110 of the
    // bounce's ~280 vector instructions less: 5 % of a depth-8 frame.
    if constexpr (LIGHTS != 0ull) if (last) {
        constexpr int l0 = __builtin_ctzll(LIGHTS);                   // (one light: its record's place is a constant)
        const int il = light_end_sig<SG, LIGHTS>(recs, mk<R>(ra.x, ra.y, ra.z), mk<R>(ra.w, rb.x, rb.y), live);
        on_light = live && il >= 0;
        light = (uint32_t)lds.sc.shapes[(LIGHTS & (LIGHTS - 1ull)) == 0ull || il < 0 ? l0 : il].pad >> 16;
        alive = false;
        capped = false;
        return;
    }
    HitRec<R> h;
    // (REC_OFFSET: the hit comes back as its record's byte offset in LeanLds::rec, the miss record's included)
    constexpr bool REC_OFFSET = LEAN_REC && lean_part(DRT_LEAN_REC_OFFSET, NP), MASK_NORMAL = LEAN_REC && lean_part(DRT_LEAN_MASK_NORMAL, NP),
                   MASK_REST = LEAN_REC && lean_part(DRT_LEAN_MASK_REST, NP);
    if constexpr (REC_OFFSET)
        h = closest_hit_sig<SG, R, SG::n * (int)sizeof(LeanRec), (int)sizeof(LeanRec)>(recs, mk<R>(ra.x, ra.y, ra.z), mk<R>(ra.w, rb.x, rb.y));
    else if constexpr (LEAN_REC)                                      // (a miss: the index of LeanLds's miss record)
        h = closest_hit_sig<SG, R, SG::n>(recs, mk<R>(ra.x, ra.y, ra.z), mk<R>(ra.w, rb.x, rb.y));
    else
        h = path_closest_hit<SG>(sc, recs, ra, rb);
    // (LEAN_REC: a miss reads the miss record -- no BxDF, no emitter -- and every use of `hit` below asks for one of the two)
    const bool hit = LEAN_REC ? live : live && h.prim >= 0;
    const int prim = LEAN_REC ? h.prim : (h.prim >= 0 ? h.prim : 0);  // (a miss reads record 0, uses nothing of it)
    const V3<R> o = mk<R>(ra.x, ra.y, ra.z);
    const V3<R> d = mk<R>(ra.w, rb.x, rb.y);
    const V3<R> P = o + d * h.t;                                      // pathtracer.hpp:83
    const DevShape<R>& sh = lds.sc.shapes[LEAN_REC ? 0 : prim];
    uint32_t ids = 0, cid, eid, crow = 0;                             // colour | emission << 16 parameter ids
    float4 lean_a = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (LEAN_REC) {
        const LeanRec& lr = REC_OFFSET ? *reinterpret_cast<const LeanRec*>(reinterpret_cast<const char*>(ll->rec) + prim) : ll->rec[prim];
        lean_a = lr.a;
        const uint2 b = lr.b;
        crow = cid = b.x;                                             // (with colour columns: the colour row's offset, not the id)
        eid = b.y;
    } else {
        ids = (uint32_t)sh.pad;
        cid = ids & 0xFFFFu;
        eid = ids >> 16;
    }
    const bool has_bxdf = cid != DRT_ID_NONE, emits = hit && eid != DRT_ID_NONE;
    // emission, pathtracer.hpp:113-114: a shape with BxDF AND emitter (rare) adds it here, a pure light is the caller's
    on_light = emits && !has_bxdf;
    light = eid;
    if (last && !vo) {
        if constexpr (!NO_LIT_BXDF) if (wave_any(emits && has_bxdf)) {
            if (emits && has_bxdf) {
                if (NP != 0 && seed_px)
                    g = mk<R>((R)seed_px[0], (R)seed_px[1], (R)seed_px[2]);
                add_emission<R, NP, NC>(lds, tl, params, eid, inv_pk, T, g, L, tg);
            }
        }
        alive = false;
        capped = false;
        if constexpr (!FIXED) if (!a.cap_is_roulette) {                // (a user max_depth: had the roulette let the path live?)
            const bool rr_kills = next_rr && draw(n_theta + 2) < a.rr_threshold;
            capped = hit && has_bxdf && !rr_kills;
        }
        return;
    }
    const V3<R> ctr = LEAN_REC ? mk<R>((R)lean_a.x, (R)lean_a.y, (R)lean_a.z) : mk<R>(sh.p[0], sh.p[1], sh.p[2]);
    // (f32: (P - c) / r with 1 / r from a table would save the rsq and the select -- and moves sphere normals by a few ulp,
    //  which flips one grazing path of the 64 x 48 x 8 smoke frame: measured, not kept; the literal form stays)
    V3<R> nsph = ctr;
    if constexpr (!MASK_NORMAL)
        nsph = normalize(P - ctr);                                    // shape.hpp:105-106
    const bool is_plane = (LEAN_REC ? __float_as_int(lean_a.w) : sh.type) == DRT_SHAPE_PLANE;   // shape.hpp:58-59: the normal as stored
    V3<R> nrm = mk<R>(is_plane ? ctr.x : nsph.x, is_plane ? ctr.y : nsph.y, is_plane ? ctr.z : nsph.z);
    if constexpr (MASK_NORMAL) {
        // the sphere's normal in the sphere's lanes alone (nrm = ctr so far): the same normalize on the same operands, no select for the
        // planes' lanes, and a wave that hit no sphere branches over it (the empty asm keeps the compiler from making selects of the
        // branch again)
        if (!is_plane) {
            V3<R> n = normalize(P - ctr);                             // shape.hpp:105-106
            asm volatile("" : "+v"(n.x), "+v"(n.y), "+v"(n.z));
            nrm = n;
        }
    }
#ifdef DRT_USER_SHAPES
    if (sh.type >= DRT_SHAPE_USER) {                                  // a caller-defined kind: its own normal(point) (shape.hpp:22)
        const R p8[8] = {sh.p[0], sh.p[1], sh.p[2], sh.p[3], lds.user_q[prim][0], lds.user_q[prim][1], lds.user_q[prim][2], lds.user_q[prim][3]};
        nrm = user_normal<R>(sh.type - DRT_SHAPE_USER, p8, P);
    }
#endif
    if (vo) {
        vo->P = P; vo->nrm = nrm; vo->d = d;
        vo->ids = ids;
        vo->material = sh.material;
        vo->hit = hit;
        vo->scattered = hit && has_bxdf;
    }
    if constexpr (!NO_LIT_BXDF) if (wave_any(emits && has_bxdf)) {
        if (emits && has_bxdf) {
            if (NP != 0 && seed_px)
                g = mk<R>((R)seed_px[0], (R)seed_px[1], (R)seed_px[2]);
            add_emission<R, NP, NC>(lds, tl, params, eid, inv_pk, T, g, L, tg);
        }
    }
    // the BxDF: sample, evaluate (pathtracer.hpp:91-111)
    const DevMaterial<R>& m = lds.sc.materials[has_bxdf ? sh.material : 0];
    V3<R> wo;
    R q, bs;
    sample_bxdf<R, SPEC>(m, nrm, d, draw(n_theta), draw(n_theta + 1), wo, q, bs);
    const R c = dot(nrm, wo);                                         // pathtracer.hpp:103
    const R mk_ = div_r(bs * c, q * pk);                              // T_{k+1} = T_k * colour * m_k (f32: v_rcp, 1 ulp)
    // roulette / cap of the next depth (pathtracer.hpp:128)
    const bool rr_kills = !FIXED && next_rr && draw(n_theta + 2) < a.rr_threshold;
    alive = hit && has_bxdf && !next_cap && !rr_kills;
    capped = !FIXED && hit && has_bxdf && next_cap && !a.cap_is_roulette && !rr_kills;
    // (live_mask, LEAN_REC: the wave's mask of `live`, of which the caller made `live` -- the mask of `alive` is then that AND the
    //  mask of a compare, on the scalar unit; a ballot of `alive` itself goes through a 0 / 1 vector register)
    if constexpr (LEAN_REC) if (live_mask)
        *live_mask &= wave_ballot(has_bxdf && !next_cap);
    // the throughput moves on only in lanes whose path goes on (the others stay frozen for the light's turn); with
    // gradients it leaves zero colour channels out and counts them, and counts the bounce for its colour (see Tangents)
    // (REST, the lockstep kernel's colour-column form: a lane that does not go on reads the table's row of ones and zero increments)
    constexpr bool REST = FREEZE_BY_ROW && NC > 0 && NP != DRT_NP_ANY && !DRT_NP_IS_DIR(NP) && NP != DRT_NP_SETS;
    // (DIR, forward mode: the same by its own table's rest row, in every form)
    constexpr bool DIR = DRT_NP_IS_DIR(NP), BY_ROW = REST || DIR;
    if constexpr (NP == DRT_NP_SETS) {
        // K parameter sets: every set's throughput moves on by its own colour row; a lane that stops reads the rest row and m = 1
        const uint32_t row = (alive && cid < tg.rest ? cid : tg.rest) * 4u;
        const R mm = alive ? mk_ : R(1);
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const R* rec = tg.tab + (uint32_t)k * tg.stride + row;
            tg.T[k] = tg.T[k] * (mk<R>(rec[0], rec[1], rec[2]) * mm);
        }
    } else if constexpr (NP == DRT_NP_SETS_ALONG) {
        // K sets, a direction each: set k's three rows -- its colour, d / c, d (zero channels) -- move its T, zc, S and Z as the forward-mode
        // form moves its own; a lane that stops reads the rest row and m = 1
        const uint32_t row = (alive && cid < tg.rest ? cid : tg.rest) * 4u;
        const R mm = alive ? mk_ : R(1);
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const R *rec = tg.tab + (uint32_t)k * tg.words + row, *ds = rec + tg.stride, *dz = ds + tg.stride;
            tg.T[k] = tg.T[k] * (mk<R>(rec[0], rec[1], rec[2]) * mm);
            tg.zc[k] += pid_unpack(rec[3]);
            tangent_advance(ds, dz, tg.S[k], tg.Z[k]);
        }
    } else if constexpr (NP == DRT_NP_SETS_GRAD) {
        // K sets, a gradient each: set k's colour row moves its T and zc as the general form moves its own; a lane that stops reads the rest
        // row and m = 1.  The vertex joins the ONE history the sets share
        const uint32_t row = (alive && cid < tg.rest ? cid : tg.rest) * 4u;
        const R mm = alive ? mk_ : R(1);
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const R* rec = tg.tab + (uint32_t)k * tg.words + row;
            tg.T[k] = tg.T[k] * (mk<R>(rec[0], rec[1], rec[2]) * mm);
            tg.zc[k] += pid_unpack(rec[3]);
        }
        tg.h.template push<true>(live, alive ? cid : 0xFFu);
    } else if constexpr (MASK_REST && REST) {
        // the colour's row of LeanLds by its offset, in the lanes that go on alone: a lane that stops would read the rest row -- a factor
        // of exactly 1, increments of 0 -- and keeps its bits without the read
        // (live_mask: the wave's mask of `alive` stands in the scalar pair already)
        // (end_ids: the caller's "which light the path ended on", moved on here, ahead of the block -- its select is the last use of the
        //  mask of `live`, which would otherwise stay in a scalar pair of its own across the block)
        if (end_ids) {
            uint32_t e = on_light ? light : *end_ids;
            asm volatile("" : "+v"(e));
            *end_ids = e;
        }
        if (live_mask ? __builtin_amdgcn_inverse_ballot_w64(*live_mask) : alive) {
            const LeanCol& lc = *reinterpret_cast<const LeanCol*>(reinterpret_cast<const char*>(ll->col) + crow);
            const float4 c4 = lc.a;
            T = T * (mk<R>((R)c4.x, (R)c4.y, (R)c4.z) * mk_);
            tg.cnt[0] += __float_as_uint(c4.w);
            if constexpr (NC > 4) {
                const uint2 b = lc.b;
                tg.cnt[NC > 4 ? 1 : 0] += b.y;
                tg.zc += b.x;
            } else
                tg.zc += lc.b.x;
        }
    } else if constexpr (LEAN_REC && REST) {
        // the colour's row of LeanLds by its offset (row 0: the rest row, for a lane that does not go on): one address, two reads
        const LeanCol& lc = *reinterpret_cast<const LeanCol*>(reinterpret_cast<const char*>(ll->col) + (alive ? crow : 0u));
        const float4 c4 = lc.a;
        const V3<R> cm = mk<R>((R)c4.x, (R)c4.y, (R)c4.z) * (alive ? mk_ : R(1));
        tg.cnt[0] += __float_as_uint(c4.w);
        if constexpr (NC > 4) {
            const uint2 b = lc.b;
            tg.cnt[NC > 4 ? 1 : 0] += b.y;
            tg.zc += b.x;
        } else
            tg.zc += lc.b.x;
        T = T * cm;
    } else {
        const int cidx = DIR ? (alive ? (int)cid : DRT_PATH_LDS_PARAMS) : (REST ? (alive ? (int)cid : DRT_TANGENT_REST) : (has_bxdf ? (int)cid : 0));
        V3<R> col;
        if constexpr (DIR && NC > 0) {
            // K directions: the colour row once, a row of v / c and of v (zero channels) per direction; a lane that stops reads the rest row
            const uint32_t row = ((uint32_t)cidx < tg.rest ? (uint32_t)cidx : tg.rest) * 4u;
            const R* rec = tg.tab + row;
            col = mk<R>(rec[0], rec[1], rec[2]);
            tg.zc += pid_unpack(rec[3]);
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const R *ds = tg.tab + (1u + 2u * k) * tg.stride + row, *dz = ds + tg.stride;
                tangent_advance(ds, dz, tg.S[k], tg.Z[k]);
            }
        } else
        if constexpr (DIR) {
            const int row = cidx < DRT_PATH_LDS_PARAMS ? cidx : DRT_PATH_LDS_PARAMS;
            const R *rec = tg.dl->colnz[row], *ds = tg.dl->dlog[row], *dz = tg.dl->dzero[row];
            col = mk<R>(rec[0], rec[1], rec[2]);
            tg.zc += pid_unpack(rec[3]);
            tangent_advance(ds, dz, tg.S, tg.Z);
        } else
        if constexpr (NP == DRT_NP_ANY) {
            const R* rec = tg.gl->colnz[cidx < DRT_PATH_LDS_PARAMS ? cidx : 0];
            col = mk<R>(rec[0], rec[1], rec[2]);
            tg.zc += alive ? pid_unpack(rec[3]) : 0u;
            if (ih)
                tg.template push<false>(alive, cid);      // (a lane on its own: only vertices the path goes on from)
            else
                tg.template push<true>(live, alive ? cid : 0xFFu);
        } else
            col = NC > 0 ? mk<R>(tl.colnz[cidx][0], tl.colnz[cidx][1], tl.colnz[cidx][2]) : load_param<R, (NP > 0)>(lds, params, cidx);
        const V3<R> cmv = col * (BY_ROW ? (alive ? mk_ : R(1)) : mk_);
        if constexpr (MASK_REST && NP == 0 && NC == 0) {
            // (forward only: T moves on in the lanes that go on alone -- a factor of exactly 1 in the others, as below)
            if (alive) {
                V3<R> Tn = T * cmv;
                asm volatile("" : "+v"(Tn.x), "+v"(Tn.y), "+v"(Tn.z));
                T = Tn;
            }
        } else {
        const V3<R> cm = BY_ROW ? cmv : mk<R>(alive ? cmv.x : R(1), alive ? cmv.y : R(1), alive ? cmv.z : R(1));
        if constexpr (REST) {
            tg.cnt[0] += tl.inc[cidx][0];
            if (NC > 4)
                tg.cnt[NC > 4 ? 1 : 0] += tl.inc[cidx][1];
            tg.zc += tl.inc[cidx][2];
        } else
        if constexpr (NC > 0 && NP != DRT_NP_ANY && !DRT_NP_IS_DIR(NP) && NP != DRT_NP_SETS) {
            tg.cnt[0] += alive ? tl.inc[cidx][0] : 0u;
            if (NC > 4)
                tg.cnt[NC > 4 ? 1 : 0] += alive ? tl.inc[cidx][1] : 0u;
            tg.zc += alive ? tl.inc[cidx][2] : 0u;
        }
        T = T * cm;
        }
    }
    const V3<R> no = P + wo * R(1e-3);                                // pathtracer.hpp:99
    ra.x = no.x; ra.y = no.y; ra.z = no.z; ra.w = wo.x;
    rb.x = wo.y; rb.y = wo.z;
}

// Camera::sample (camera.hpp:51-60) of sample `sl` of the lane's pixel
// ARGS_F32: the camera's constants come as the floats the host made of them (PathArgs::eye_f ...: scalar registers, re-loaded from the
// kernel's arguments where the compiler runs out of them).  Left to itself the compiler converts the double arguments with v_cvt_f32_f64,
// whose result is a VECTOR register: seventeen wave-uniform values lived through the whole kernel that way (eleven of them in scratch once
// the lockstep kernel was compiled for seven waves per SIMD).  Config 3's frame: 0.666 -> 0.659 ms, an albedo per shape 0.733 -> 0.725.  The
// regenerating form, whose scalar registers are all taken, keeps the conversions (0.353 against 0.360 ms with the arguments, which it
// re-loads in every iteration; from a table in LDS: 0.357, and the lockstep kernel 0.675).
#ifndef DRT_CAMERA_ARGS_F32
#define DRT_CAMERA_ARGS_F32 1
#endif
template <typename R, bool ARGS_F32 = (DRT_CAMERA_ARGS_F32 != 0)>
__device__ inline uint32_t path_camera(const PathArgs& a, const CameraLane<R>& cl, uint32_t gpix, uint32_t px, uint32_t py, uint32_t sl,
                                       typename Q4<R>::T& ra, typename Q2<R>::T& rb)
{
    const uint64_t path = (uint64_t)gpix * (uint64_t)a.spp + (uint64_t)(a.s0 + sl);
    const uint32_t key = (uint32_t)path;
    if (sizeof(R) == 4) {
        const float cs_step = ARGS_F32 ? a.cs_step_f : (float)(2. * a.aspect * a.tan_half * a.inv_W);
        const float ct_step = ARGS_F32 ? a.ct_step_f : (float)(2. * a.tan_half * a.inv_H);
        const V3<float> eye = ARGS_F32 ? mk<float>(a.eye_f[0], a.eye_f[1], a.eye_f[2]) : mk<float>((float)a.eye[0], (float)a.eye[1], (float)a.eye[2]);
        const V3<float> fw = ARGS_F32 ? mk<float>(a.fwd_f[0], a.fwd_f[1], a.fwd_f[2]) : mk<float>((float)a.fwd[0], (float)a.fwd[1], (float)a.fwd[2]);
        const V3<float> rt = ARGS_F32 ? mk<float>(a.right_f[0], a.right_f[1], a.right_f[2]) : mk<float>((float)a.right[0], (float)a.right[1], (float)a.right[2]);
        const V3<float> upv = ARGS_F32 ? mk<float>(a.up_f[0], a.up_f[1], a.up_f[2]) : mk<float>((float)a.up[0], (float)a.up[1], (float)a.up[2]);
        const float cs = fmaf(u01(0.f, rng_draw(a.rng_stream, key, 0)), cs_step, (float)cl.cs0);
        const float ct = fmaf(u01(0.f, rng_draw(a.rng_stream, key, 1)), ct_step, (float)cl.ct0);
        const V3<float> dir = mk<float>(fw.x + cs * rt.x - ct * upv.x, fw.y + cs * rt.y - ct * upv.y, fw.z + cs * rt.z - ct * upv.z);
        const V3<float> dn = normalize(dir);
        ra.x = (R)eye.x; ra.y = (R)eye.y; ra.z = (R)eye.z; ra.w = (R)dn.x;
        rb.x = (R)dn.y; rb.y = (R)dn.z;
    } else {                                          // f64 verification mode: the reference's own sequence, in double
        const double u1 = (double)rng_draw(a.rng_stream, key, 0) / DRT_RAND_MAX_D;
        const double u2 = (double)rng_draw(a.rng_stream, key, 1) / DRT_RAND_MAX_D;
        const double s = ((double)px + u1) / (double)a.W;
        const double t = ((double)py + u2) / (double)a.H;
        const double cs = (2. * s - 1.) * a.aspect * a.tan_half;
        const double ct = (2. * t - 1.) * a.tan_half;
        double dx = a.fwd[0] + cs * a.right[0] - ct * a.up[0];
        double dy = a.fwd[1] + cs * a.right[1] - ct * a.up[1];
        double dz = a.fwd[2] + cs * a.right[2] - ct * a.up[2];
        const double inv = 1.0 / sqrt(dx * dx + dy * dy + dz * dz);
        ra.x = (R)a.eye[0]; ra.y = (R)a.eye[1]; ra.z = (R)a.eye[2]; ra.w = (R)(dx * inv);
        rb.x = (R)(dy * inv); rb.y = (R)(dz * inv);
    }
    return key;
}
// ... of sample `sl` of pixel `gpix`, for a lane that is not bound to one pixel (k_path's regenerating form): `cl` holds that
// pixel's constants; the f64 mode needs the pixel's coordinates too
template <typename R>
__device__ inline uint32_t path_camera(const PathArgs& a, const CameraLane<R>& cl, uint32_t gpix, uint32_t sl,
                                       typename Q4<R>::T& ra, typename Q2<R>::T& rb)
{
    uint32_t px = 0, py = 0;
    if (sizeof(R) != 4) {
        py = gpix / (uint32_t)a.W;
        px = gpix - py * (uint32_t)a.W;
    }
    return path_camera<R, false>(a, cl, gpix, px, py, sl, ra, rb);
}
// ... of k_path_lean beside a compiled-in program (f32; a twin, so that path_camera keeps its text for every other kernel): the same camera,
// its two draws by the sample's folded key (drt_fold.h), which it makes here, once, and leaves in `kf` for the draws of the sample's bounces
// (path_bounce: FOLDED).  The same draws bit for bit -- tests/cpp/fold_kat.cpp -- and so the same ray.
template <bool ARGS_F32>
__device__ inline uint32_t path_camera_folded(const PathArgs& a, const CameraLane<float>& cl, uint32_t gpix, uint32_t sl, float4& ra, float2& rb, uint32_t& kf)
{
    const uint64_t path = (uint64_t)gpix * (uint64_t)a.spp + (uint64_t)(a.s0 + sl);
    const uint32_t key = (uint32_t)path;
    kf = fold16(key);
    const float cs_step = ARGS_F32 ? a.cs_step_f : (float)(2. * a.aspect * a.tan_half * a.inv_W);
    const float ct_step = ARGS_F32 ? a.ct_step_f : (float)(2. * a.tan_half * a.inv_H);
    const V3<float> eye = ARGS_F32 ? mk<float>(a.eye_f[0], a.eye_f[1], a.eye_f[2]) : mk<float>((float)a.eye[0], (float)a.eye[1], (float)a.eye[2]);
    const V3<float> fw = ARGS_F32 ? mk<float>(a.fwd_f[0], a.fwd_f[1], a.fwd_f[2]) : mk<float>((float)a.fwd[0], (float)a.fwd[1], (float)a.fwd[2]);
    const V3<float> rt = ARGS_F32 ? mk<float>(a.right_f[0], a.right_f[1], a.right_f[2]) : mk<float>((float)a.right[0], (float)a.right[1], (float)a.right[2]);
    const V3<float> upv = ARGS_F32 ? mk<float>(a.up_f[0], a.up_f[1], a.up_f[2]) : mk<float>((float)a.up[0], (float)a.up[1], (float)a.up[2]);
    const float cs = fmaf(u01(0.f, combine_folded(fold16(drt_rng_index_hash(a.rng_stream, 0)), kf)), cs_step, (float)cl.cs0);
    const float ct = fmaf(u01(0.f, combine_folded(fold16(drt_rng_index_hash(a.rng_stream, 1)), kf)), ct_step, (float)cl.ct0);
    const V3<float> dir = mk<float>(fw.x + cs * rt.x - ct * upv.x, fw.y + cs * rt.y - ct * upv.y, fw.z + cs * rt.z - ct * upv.z);
    const V3<float> dn = normalize(dir);
    ra.x = eye.x; ra.y = eye.y; ra.z = eye.z; ra.w = dn.x;
    rb.x = dn.y; rb.y = dn.z;
    return key;
}

// blocks per CU (= waves per SIMD) a k_path instantiation is compiled for (its register budget); the knobs are above.
// A kernel hiprtc makes for a scene of MANY shapes (their records in scalar registers, their tests unrolled) needs the registers: rooms of
// 15 / 31 shapes, 4 parameters, ms per launch on config 3's frame at six waves with converted constants / seven / six with the constants as
// arguments / seven with them: 0.858 / 0.849 / 0.847 / 1.039 and 2.21 / 2.50 / 2.37 / 2.61 -- so the seventh wave and the float arguments
// (path_camera) are for kernels of up to DRT_LEAN_MAX_SHAPES compiled-in shapes (the reference's scene has 9) and for the run-time program.
// Kernels that carry caller-defined kinds (DRT_USER_SHAPES: the caller's own intersect / normal / BxDF bodies inlined) keep the wider budgets too:
// a power-cosine lobe from source lost 5-8 % at six waves (1.84 -> 1.93 ms, with a disc 1.94 -> 2.09).
#ifndef DRT_LEAN_MAX_SHAPES
#ifdef DRT_USER_SHAPES
#define DRT_LEAN_MAX_SHAPES (-1)
#else
#define DRT_LEAN_MAX_SHAPES 10
#endif
#endif
template <size_t RB, bool SPEC, int NP, int NSG, bool REGEN, int NCR = 0>
constexpr int path_min_blocks()
{
    if (NP == DRT_NP_SETS_GRAD)    // K parameter sets with a gradient each, lockstep: the general form + seven values per set (f64: what the largest tables leave)
        return RB == 4 ? (DRT_NC_OF(NCR) <= 2 ? DRT_SETS_GRAD2_MIN_BLOCKS : (DRT_NC_OF(NCR) <= 4 ? DRT_SETS_GRAD4_MIN_BLOCKS : DRT_SETS_GRAD8_MIN_BLOCKS))
                       : (DRT_NC_OF(NCR) <= 2 ? 2 : 1);
    if (NP == DRT_NP_SETS_ALONG)   // K parameter sets with a direction each, lockstep: sixteen values and six fp64 sums per set beside the forward-only kernel's
        return RB == 4 ? (DRT_NC_OF(NCR) <= 2 ? DRT_SETS_ALONG2_MIN_BLOCKS : DRT_SETS_ALONG4_MIN_BLOCKS) : (DRT_NC_OF(NCR) <= 2 && !SPEC ? 2 : 1);
    if (NP == DRT_NP_SETS)         // K parameter sets, lockstep: six values and three fp64 sums per set beside the forward-only kernel's
        return RB == 4 ? (DRT_NC_OF(NCR) <= 2 ? DRT_SETS2_MIN_BLOCKS : (DRT_NC_OF(NCR) <= 4 ? DRT_SETS4_MIN_BLOCKS : DRT_SETS8_MIN_BLOCKS))
                       : (DRT_NC_OF(NCR) <= 2 ? (SPEC ? 2 : 3) : (DRT_NC_OF(NCR) <= 4 ? 2 : 1));
    if (NP == DRT_NP_CROSS)        // K directions with the samples' cross moments, lockstep: 3 K + 3 more fp64 sums beside the K-direction form's
        return RB == 4 ? (DRT_NC_OF(NCR) <= 2 ? DRT_CROSS2_MIN_BLOCKS : (DRT_NC_OF(NCR) <= 4 ? (SPEC ? 2 : DRT_CROSS4_MIN_BLOCKS) : DRT_CROSS8_MIN_BLOCKS))
                       : (DRT_NC_OF(NCR) <= 2 ? 2 : 1);
    if (NP == DRT_NP_TANGENT && DRT_NC_OF(NCR) > 0)   // K directions, lockstep: f64 takes what a block per CU has
        return RB == 4 ? (DRT_NC_OF(NCR) <= 2 ? DRT_TANGENTS2_MIN_BLOCKS : (DRT_NC_OF(NCR) <= 4 ? DRT_TANGENTS4_MIN_BLOCKS : DRT_TANGENTS8_MIN_BLOCKS))
                       : (DRT_NC_OF(NCR) <= 2 ? 2 : 1);
    if (NP == DRT_NP_TANGENT)      // forward mode: the forward-only kernel + ten values per lane (S, Z, dL, zc) and 8 / 16 KB of LDS (f32 / f64)
        return RB == 4 ? (REGEN ? DRT_TANGENT_REGEN_MIN_BLOCKS : DRT_TANGENT_MIN_BLOCKS) : ((REGEN || SPEC) ? 2 : DRT_TANGENT_F64_MIN_BLOCKS);
    if (RB == 4 && NP <= 4) {
        if (!REGEN)
            return SPEC ? ((NP == DRT_NP_ANY || NSG > DRT_LEAN_MAX_SHAPES) ? 5 : DRT_LOCKSTEP_SPEC_MIN_BLOCKS)
                        : (NP == DRT_NP_ANY ? DRT_LOCKSTEP_GEN_MIN_BLOCKS : (NSG <= DRT_LEAN_MAX_SHAPES ? DRT_LOCKSTEP_MIN_BLOCKS : DRT_LOCKSTEP_GEN_MIN_BLOCKS));
        return (NP == DRT_NP_ANY && NSG == 0) ? 4             // (general form + the kind-sorted program: 34 KB of LDS)
                                              : (SPEC ? 5 : DRT_REGEN_MIN_BLOCKS);
    }
    return (RB == 8 && NP <= 4 && !REGEN && !SPEC) ? DRT_F64_MIN_BLOCKS : 1;
}

// ---- what the entry points share: k_path, k_path_sets_cross, k_path_lean, k_path_unbiased (below) and k_path_mesh (drt_path_mesh.h) ----
// Prologue and epilogue of a launch whose wave is (pixel group, sample range), written once.  None of these functions knows its caller.
// The kernels keep their own __shared__ declarations, in their own order -- the order of the LDS symbols is part of a kernel's code -- and
// hand them in by reference.

// the finishing kernel behind a path launch adds into total[0..7]: the launch's first block zeroes them
__device__ inline void zero_totals(unsigned long long* __restrict__ total)
{
    if (total && blockIdx.x == 0 && threadIdx.x < 8)
        total[threadIdx.x] = 0;
}

// where a lane stands in the launch: its wave's pixel group and sample range
struct PathLane {
    uint32_t lane, w;          // lane of the wave; wave of the grid = group + n_groups * range
    uint32_t range, lp;        // the wave's sample range; batch-local pixel of this lane
    bool have;                 // the range and the pixel exist
    uint32_t s_begin, s_end;   // the range's samples
};
__device__ inline PathLane path_lane(const PathArgs& a)
{
    PathLane pl;
    pl.lane = threadIdx.x & (DRT_WAVE - 1);
    pl.w = grid_wave();
    pl.range = pl.w / a.n_groups;
    const uint32_t group = pl.w - pl.range * a.n_groups;
    pl.lp = group * DRT_WAVE + pl.lane;
    pl.have = pl.range < a.n_ranges && pl.lp < a.Pb;
    pl.s_begin = pl.range * a.spr;
    pl.s_end = pl.s_begin + a.spr < a.Sb ? pl.s_begin + a.spr : a.Sb;
    return pl;
}
// ... in a launch that holds several frames (k_path_views): `w` is the wave's place in its own frame's grid.  (A function of its own: with
// the wave as a defaulted argument of path_lane, 62 instantiations of the kernels above scheduled their prologues differently.)
__device__ inline PathLane path_lane_in_frame(const PathArgs& a, uint32_t w)
{
    PathLane pl;
    pl.lane = threadIdx.x & (DRT_WAVE - 1);
    pl.w = w;
    pl.range = pl.w / a.n_groups;
    const uint32_t group = pl.w - pl.range * a.n_groups;
    pl.lp = group * DRT_WAVE + pl.lane;
    pl.have = pl.range < a.n_ranges && pl.lp < a.Pb;
    pl.s_begin = pl.range * a.spr;
    pl.s_end = pl.s_begin + a.spr < a.Sb ? pl.s_begin + a.spr : a.Sb;
    return pl;
}
// f32: the pixel's corner in double ONCE per lane; a sample then only adds its jitter (camera.hpp:53-58 in the form
// cs = cs0 + u1 (2 aspect tan / W)): the sample's position inside the pixel is exact to ~2e-5 of a pixel and the
// direction to 1 ulp of f32 -- the resolution the ray has anyway once it is stored in f32
template <typename R>
__device__ inline CameraLane<R> camera_lane(const PathArgs& a, uint32_t px, uint32_t py)
{
    CameraLane<R> cl;
    cl.cs0 = (R)((2. * (double)px * a.inv_W - 1.) * a.aspect * a.tan_half);
    cl.ct0 = (R)((2. * (double)py * a.inv_H - 1.) * a.tan_half);
    return cl;
}

// Does the kernel take the camera's and the roulette's constants as the floats among its arguments (see path_camera)?  The lockstep f32
// kernels of few compiled-in shapes; not the kernels whose lanes stand at their own depths (REGEN; k_path_mesh), whose scalar registers are taken.
template <typename R, typename SG, bool REGEN = false>
constexpr bool path_args_f32()
{
    return sizeof(R) == 4 && !REGEN && DRT_CAMERA_ARGS_F32 != 0 && SG::n <= DRT_LEAN_MAX_SHAPES;
}
// three rows of a [range][row][pixel] array of Pb pixels a row, from the lane's place in the first of them: coalesced over the wave
template <typename T>
__device__ inline void store_rows3(double* f, uint32_t Pb, T x, T y, T z)
{
    f[0] = (double)x; f[(size_t)Pb] = (double)y; f[(size_t)Pb * 2] = (double)z;
}
// the wave's segments and the paths a user cap cut short, for the finishing kernel: counts[row][wave of the grid]
__device__ inline void store_counts(const PathArgs& a, const PathLane& pl, uint32_t* __restrict__ counts, uint32_t n_seg, uint32_t n_capped)
{
    if (pl.lane == 0) {
        counts[pl.w] = n_seg;
        counts[(size_t)a.n_groups * a.n_ranges + pl.w] = n_capped;
    }
}

// Block reduction of the gradient columns in fp64: thread -> wave (shuffles) -> block (LDS: `red`, the kernel's own), fixed order; thread r
// writes row r of the block's sums to its row of gpart (rows >= 3 NP: 0) and the finishing kernel adds the blocks.  The columns are the ones
// the lanes keep in LDS (Tangents::acc: row r of this thread at acc[r * DRT_BLOCK]).  (Always inline: at eight parameters the compiler
// otherwise leaves it a call, with a stack pointer, in k_path_mesh.)
template <int NP, typename R>
__device__ __forceinline__ void block_grad_sums(const R* acc, double (*red)[DRT_FAST_PARAMS * 3], double* gpart, uint32_t lane)
{
    const int wv = threadIdx.x / DRT_WAVE;
#pragma unroll
    for (int r = 0; r < NP * 3; ++r) {
        double v = (double)acc[r * DRT_BLOCK];
#pragma unroll
        for (int o2 = DRT_WAVE / 2; o2 > 0; o2 >>= 1)
            v += __shfl_down(v, o2);
        if (lane == 0)
            red[wv][r] = v;
    }
    __syncthreads();
    if (threadIdx.x < DRT_FAST_PARAMS * 3) {
        double v = 0;
        if ((int)threadIdx.x < NP * 3)
            for (int ww = 0; ww < DRT_BLOCK / DRT_WAVE; ++ww)
                v += red[ww][threadIdx.x];
        gpart[(size_t)blockIdx.x * (DRT_FAST_PARAMS * 3) + threadIdx.x] = v;
    }
}

// ---- the kernel -----------------------------------------------------------------------------------
// The bounce loop is written WITHOUT per-lane branches: every lane of the wave executes every bounce of the sample --
// a lane whose path has ended keeps tracing a stale ray whose results are never used (`live` guards every
// accumulation, its T and dT are frozen by selects) -- because that is what the SIMD does anyway, and straight-line
// code spares the exec-mask bookkeeping, the register copies at the joins and the waits in front of them.
// REGEN = false: all lanes of a wave trace their pixel's sample s at the same time and stand at the same depth (scalar
// depth bookkeeping; lanes whose path ended idle to the end of the sample: fine when paths end at a fixed depth).
// REGEN = true: every lane is on its own -- when its path ends (the roulette of pathtracer.hpp:128 ends paths at any
// depth) it starts its next sample at once, so no lane waits for the longest path of the wave: per-lane depth
// bookkeeping, the camera code runs whenever some lane starts over, the light's emission is added when the lane's
// path ends.  ~35 % more instructions per bounce, but roulette-terminated renders (the reference's defaults, -b 1
// -p 0.5: 2.5 vertices per path on average, some paths 20) keep their lanes busy.
// (waves per SIMD by form: path_min_blocks above)
// (NCR: the colour columns NC and, above its low byte, the slots' roles -- DRT_NC_ROLES)
template <typename R, bool SPEC, int NP, int NCR, typename SG, bool REGEN = false, bool LOSS = false>
__global__ void __launch_bounds__(DRT_BLOCK, (path_min_blocks<sizeof(R), SPEC, NP, SG::n, REGEN, NCR>()))
k_path(PathArgs a, const DevScene<R>* __restrict__ sc, const R* __restrict__ params, const float* __restrict__ adjoint,
       double* __restrict__ gpart, double* __restrict__ fpart, uint32_t* __restrict__ counts,
       unsigned long long* __restrict__ total, double* __restrict__ gimg_part
#ifdef DRT_SAMPLE_LOSS
       , LossValues loss_lv, double* __restrict__ loss_part     // loss_part[wave of the grid]: the sum of the values of the wave's samples
#endif
       )
{
    zero_totals(total);
    typedef typename Q4<R>::T R4;
    typedef typename Q2<R>::T R2;
    constexpr int NC = DRT_NC_OF(NCR), ROLES = DRT_ROLES_OF(NCR);
#ifdef DRT_SAMPLE_LOSS
    R loss_q[DRT_MAX_LOSS_VALUES];
#pragma unroll
    for (int k = 0; k < DRT_MAX_LOSS_VALUES; ++k)
        loss_q[k] = (R)loss_lv.q[k];
    double loss_sum = 0.0;                                // this lane's sum of value_s over the samples it finished
#endif
    constexpr bool JAC = DRT_JACOBIAN_OF(NCR) && NP > 0 && !REGEN;   // the Jacobian form: every row of the lane's column leaves per pixel
    __shared__ PathSceneLds<R> lds;
    __shared__ double s_red[REGEN ? 1 : DRT_BLOCK / DRT_WAVE][DRT_FAST_PARAMS * 3];   // (REGEN: the block's gradient partials reuse the pixel sums' table)
    __shared__ TangentLds<R> s_tl;
    constexpr bool GEN = NP == DRT_NP_ANY;                // any number of parameters: history + per-wave tables (see Tangents<R, DRT_NP_ANY>)
    constexpr bool SGRAD = NP == DRT_NP_SETS_GRAD;        // one path under NC parameter sets, a summed gradient each: the general form's block, shared history (see Tangents<R, DRT_NP_SETS_GRAD>)
    static_assert(!(SGRAD && (REGEN || NC < 1)), "the parameter-set gradient form is a lockstep form of K >= 1 sets: a lane is a pixel");
    __shared__ typename PickT<(GEN || SGRAD), GenBlock<R>, NoLds>::T s_gen;
    extern __shared__ uint32_t s_hist[];                  // GEN: [a.hist_lds][DRT_BLOCK] history words
    constexpr bool CROSS = NP == DRT_NP_CROSS;            // the K-direction form + the samples' cross moments (see Tangents<R, DRT_NP_CROSS>)
    static_assert(!(CROSS && (REGEN || NC < 1)), "the cross-moment form is a lockstep form of K >= 1 directions: a lane is a pixel");
    constexpr bool DIR = DRT_NP_IS_DIR(NP);               // forward mode: the derivative along one direction (see DirLds); `params` = [params | direction]
    constexpr bool DIRS = DIR && NC > 0;                  // ... along NC directions at once: tables in dynamic shared memory (see stage_dirs)
    static_assert(!(DIRS && REGEN), "the K-direction form is a lockstep form: a lane is a pixel");
    constexpr bool SETS = NP == DRT_NP_SETS;              // one path under NC parameter sets: tables in dynamic shared memory (see stage_sets)
    static_assert(!(SETS && (REGEN || NC < 1)), "the parameter-set form is a lockstep form of K >= 1 sets: a lane is a pixel");
    constexpr bool ALONG = NP == DRT_NP_SETS_ALONG;       // ... each set with a direction of its own (see stage_sets_along)
    static_assert(!(ALONG && (REGEN || NC < 1)), "the parameter-set form with directions is a lockstep form of K >= 1 sets: a lane is a pixel");
    __shared__ typename PickT<(DIR && !DIRS), DirLds<R>, NoLds>::T s_dir;
    if constexpr (GEN || SGRAD)
        gen_zero(s_gen);
    stage_path_scene(lds, sc, params);
    const TangentLds<R>& tl = s_tl;
    if (NC > 0 && !GEN && !DIR && !SETS && !ALONG && !SGRAD)
        stage_tangents(s_tl, lds);

    const PathLane pl = path_lane(a);

    Tangents<R, NP, NC> tg;
    __shared__ R s_acc[NP > 0 ? NP * 3 : 1][DRT_BLOCK];
    if constexpr (!SETS && !ALONG && !SGRAD)
        tg.acc = &s_acc[0][threadIdx.x];
    if constexpr (GEN)
        gen_begin(s_gen, lds, sc, a, s_hist, reinterpret_cast<uint32_t*>(a.hist_ovf), tg);
    else if constexpr (SGRAD)
        sets_grad_begin(s_gen, lds, sc, params, a, tg);
    else if constexpr (DIRS || SETS || ALONG)
        path_tables_begin(tg, lds, params);
    else if constexpr (DIR) {
        stage_dir(s_dir, lds, params);
        tg.dl = &s_dir;
        tg.new_path();
    } else {
#pragma unroll
        for (int p = 0; p < NP; ++p)
            tg.acc_set(p, mk<R>(R(0), R(0), R(0)));
    }
    double fx = 0, fy = 0, fz = 0;                        // radiance sum of this lane's pixel over the range
    double tx = 0, ty = 0, tz = 0;                        // DIR: ... and the sum of its samples' derivatives
    constexpr int TK = ALONG ? 2 : 1;                     // rows of three sums a direction / a set has (the write-out below)
    // (tk's size and zeroing stay spelled per form: as TK * NC and one loop over it they moved 16 kernels' instruction streams)
    double tk[(DIRS || SETS) ? NC : (ALONG ? 2 * NC : 1)][3];   // DIRS: ... per direction; SETS: the radiance sums per set; ALONG: radiance, derivative per set
    if constexpr (DIRS || SETS || ALONG) {
#pragma unroll
        for (int k = 0; k < (ALONG ? 2 * NC : NC); ++k)
            tk[k][0] = tk[k][1] = tk[k][2] = 0.0;
    }
    if constexpr (CROSS) {
#pragma unroll
        for (int k = 0; k < NC; ++k)
            tg.Q[k][0] = tg.Q[k][1] = tg.Q[k][2] = 0.0;
        tg.S2[0] = tg.S2[1] = tg.S2[2] = 0.0;
    }
    uint32_t n_seg = 0, n_capped = 0;                     // wave-uniform counters

    uint32_t gpix = 0, px = 0, py = 0;
    V3<R> g = mk<R>(R(1), R(1), R(1));                    // render.cpp:80: radiance.backward(Vec3(1))
    if (pl.have) {
        gpix = path_global_pixel(a, a.p0 + pl.lp);
        py = gpix / (uint32_t)a.W;
        px = gpix - py * (uint32_t)a.W;
        if (NP != 0 && adjoint)
            g = mk<R>((R)adjoint[(size_t)gpix * 3], (R)adjoint[(size_t)gpix * 3 + 1], (R)adjoint[(size_t)gpix * 3 + 2]);
        if constexpr (SGRAD) if (adjoint) {
            // a seed per set: the caller's n_sets images, one behind the other
#pragma unroll
            for (int k = 0; k < NC; ++k)
                if ((uint32_t)k < tg.n_sets) {
                    const float* gk = adjoint + ((size_t)k * (size_t)a.W * (size_t)a.H + gpix) * 3;
                    tg.g[k] = mk<R>((R)gk[0], (R)gk[1], (R)gk[2]);
                }
        }
    }
    const CameraLane<R> cl = camera_lane<R>(a, px, py);
    constexpr bool ARGS_F32 = path_args_f32<R, SG, REGEN>();
    const R pk_rr = ARGS_F32 ? (R)a.p_rr_f : (R)a.p_rr, inv_p_rr = ARGS_F32 ? (R)a.inv_p_rr_f : (R)a.inv_p_rr;
    ProgRecs<SG::n, R> recs;
    // (the kind-sorted program's 1.3 KB only where it runs: with the kinds compiled in they are what stands between the
    //  regenerating kernel and a sixth block per CU)
    __shared__ typename PickT<(SG::n == 0), ProgLds, NoLds>::T s_prog;
    recs.lds = reinterpret_cast<const ProgLds*>(&s_prog);
    if (SG::n > 0)
        recs.template load<SG>(sc);
    if constexpr (sizeof(R) == 4 && SG::n == 0) {
        const DevScene<float>* scf = reinterpret_cast<const DevScene<float>*>(sc);
        if (threadIdx.x < DRT_PROG_SORTED_MAX) {
            s_prog.rec[threadIdx.x] = *reinterpret_cast<const float4*>(scf->sorted[threadIdx.x]);
            s_prog.shape[threadIdx.x] = scf->sorted_shape[threadIdx.x];
        }
        if (threadIdx.x < 8)
            s_prog.kind_begin[threadIdx.x] = scf->kind_begin[threadIdx.x];
        __syncthreads();
    }

    if (pl.range < a.n_ranges && !REGEN) {
    for (uint32_t sl = pl.s_begin; sl < pl.s_end; ++sl) {
        R4 ra;
        R2 rb;
        const uint32_t key = path_camera<R, ARGS_F32>(a, cl, gpix, px, py, sl, ra, rb);
        // pathtracer.hpp:128 at depth 0
        bool live = pl.have && a.depth_cap > 0 && !(a.min_bounces <= 0 && rng_draw(a.rng_stream, key, 2) < a.rr_threshold);
        V3<R> T = mk<R>(R(1), R(1), R(1)), L = mk<R>(R(0), R(0), R(0));
        uint32_t end_ids = DRT_ID_NONE;                   // emission parameter of the light the path ended on
        R end_inv_pk = R(1);
        if (NC > 0 || GEN || DIR)
            tg.new_path();
        for (int kk = 0; kk < a.depth_cap; ++kk) {
            const uint32_t n_live = (uint32_t)__popcll(wave_ballot(live));
            if (n_live == 0)
                break;
            n_seg += n_live;
            const R pk = kk >= a.min_bounces ? pk_rr : R(1);                  // pathtracer.hpp:130
            const R inv_pk = kk >= a.min_bounces ? inv_p_rr : R(1);
            const uint32_t n_theta = draw_offset(kk, 0, a.min_bounces) + camera_draw_base(a.min_bounces);
            const bool next_rr = (kk + 1) >= a.min_bounces;
            const bool next_cap = (kk + 1) >= a.depth_cap;
            bool alive, capped, on_light;
            uint32_t light;
            // (the row of ones for lanes that stop: measured on the diffuse f32 kernels of few shapes, theirs alone)
            path_bounce<R, SPEC, NP, NC, SG, (DRT_FREEZE_BY_ROW != 0 && sizeof(R) == 4 && !SPEC && SG::n <= DRT_LEAN_MAX_SHAPES)>(a, lds, tl, sc, params, recs, key, pk, inv_pk, n_theta, next_rr, next_cap, live, g,
                                                    ra, rb, T, L, tg, alive, capped, on_light, light, nullptr, next_cap);
            // A light without a BxDF ends the path: T and dT stay as they are in this lane, so its emission is added
            // ONCE PER SAMPLE, after the bounce loop, for all lanes together -- not here, where every bounce a few lanes
            // of the wave would drag the other sixty through it.
            end_ids = on_light ? light : end_ids;
            end_inv_pk = on_light ? inv_pk : end_inv_pk;
            if (next_cap && !a.cap_is_roulette)
                n_capped += (uint32_t)__popcll(wave_ballot(capped));
            live = alive;
        }
        if (wave_any(end_ids != DRT_ID_NONE)) {
            if (end_ids != DRT_ID_NONE)
                add_emission<R, NP, NC, LOSS, PathSceneLds<R>, ROLES>(lds, tl, params, end_ids, end_inv_pk, T, g, L, tg
#ifdef DRT_SAMPLE_LOSS
                                                                      , loss_q
#endif
                                                                      );
        }
#ifdef DRT_SAMPLE_LOSS
        if (LOSS && pl.have) {
            // L is final: no shape of the scenes this form takes both scatters and emits.  A path that reached no light counts with L = 0.
            R value_ = R(0);
            V3<R> seed_ = mk<R>(R(0), R(0), R(0));
            sample_loss<R>(loss_q, L, g, value_, seed_);
            loss_sum += (double)value_;
        }
#endif
        if constexpr (ALONG) {
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                tk[2 * k][0] += (double)tg.L[k].x; tk[2 * k][1] += (double)tg.L[k].y; tk[2 * k][2] += (double)tg.L[k].z;
                tk[2 * k + 1][0] += (double)tg.dL[k].x; tk[2 * k + 1][1] += (double)tg.dL[k].y; tk[2 * k + 1][2] += (double)tg.dL[k].z;
            }
        } else
        if constexpr (SETS) {
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                tk[k][0] += (double)tg.L[k].x; tk[k][1] += (double)tg.L[k].y; tk[k][2] += (double)tg.L[k].z;
            }
        } else {
            fx += (double)L.x; fy += (double)L.y; fz += (double)L.z;
        }
        if constexpr (DIRS) {
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                tk[k][0] += (double)tg.dL[k].x; tk[k][1] += (double)tg.dL[k].y; tk[k][2] += (double)tg.dL[k].z;
            }
        } else
        if constexpr (DIR) {
            tx += (double)tg.dL.x; ty += (double)tg.dL.y; tz += (double)tg.dL.z;
        }
        if constexpr (CROSS) {
            // the sample's products, from its own values: Q_k += dL_k L, S2 += L L
            const double lx = (double)L.x, ly = (double)L.y, lz = (double)L.z;
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                tg.Q[k][0] += (double)tg.dL[k].x * lx; tg.Q[k][1] += (double)tg.dL[k].y * ly; tg.Q[k][2] += (double)tg.dL[k].z * lz;
            }
            tg.S2[0] += lx * lx; tg.S2[1] += ly * ly; tg.S2[2] += lz * lz;
        }
    }
    }
    // ---- REGEN: a wave owns 64 pixels x its sample range, and its LANES are not bound to pixels: a lane whose path has ended
    // takes the NEXT camera sample of the wave (item n = pixel n % 64, sample n / 64: wave-uniform counter + the lane's rank
    // among the takers), so all 64 lanes stay busy until the wave's samples run out -- with a lane = a pixel the wave lasted as
    // long as its unluckiest lane's 32 paths (82 bounces where the mean lane has 62 under the reference's -b 1 -p 0.5: a
    // quarter of the wave-time idle).  What belongs to a PIXEL -- camera constants, radiance sum -- therefore
    // lives in per-wave tables in LDS (slot = the pixel's lane of the static layout, which also writes the sums out at the
    // end); radiance is added there with ds_add_f64.  (The sums of f32 values in f64 are exact unless a pixel's samples span
    // more than 2^24 in magnitude, so their order does not show; gradient sums are per lane and summed over lanes anyway.)
    __shared__ R s_pcs[REGEN ? DRT_BLOCK : 1], s_pct[REGEN ? DRT_BLOCK : 1];
    __shared__ uint32_t s_pgpix[REGEN ? DRT_BLOCK : 1];
    __shared__ double s_film[REGEN ? 3 : 1][REGEN ? DRT_BLOCK : 1];
    __shared__ uint32_t s_ih[REGEN ? DRT_DRAW_TABLE : 1];      // h(n) of every draw index a path of <= DRT_MAX_DEPTH vertices can reach
    __shared__ double s_tfilm[REGEN && DIR ? 3 : 1][REGEN && DIR ? DRT_BLOCK : 1];   // DIR: the pixels' derivative sums, like s_film
    if constexpr (REGEN && DIR) {
        s_tfilm[0][threadIdx.x] = 0.0; s_tfilm[1][threadIdx.x] = 0.0; s_tfilm[2][threadIdx.x] = 0.0;
    }
    if (REGEN) {
        for (uint32_t n = threadIdx.x; n < DRT_DRAW_TABLE; n += DRT_BLOCK)
            s_ih[REGEN ? n : 0] = drt_rng_index_hash(a.rng_stream, n);
        s_pcs[threadIdx.x] = cl.cs0;
        s_pct[threadIdx.x] = cl.ct0;
        s_pgpix[threadIdx.x] = pl.have ? gpix : 0xFFFFFFFFu;       // (no such pixel: its samples are skipped)
        s_film[0][threadIdx.x] = 0.0; s_film[REGEN ? 1 : 0][threadIdx.x] = 0.0; s_film[REGEN ? 2 : 0][threadIdx.x] = 0.0;
        __syncthreads();
    }
    if (pl.range < a.n_ranges && REGEN) {
        const uint32_t wbase = threadIdx.x & ~(uint32_t)(DRT_WAVE - 1);      // this wave's first slot in the pixel tables
        const uint32_t n_items = DRT_WAVE * (pl.s_end - pl.s_begin);
        uint32_t n_next = 0;                              // wave-uniform: the next camera sample of the wave to hand out
        uint32_t key = 0, pix = wbase, pgpix = 0;         // RNG key, pixel slot and pixel of the lane's current path
        int kk = 0;                                       // depth of the lane's current path
        bool live = false;
        R4 ra;
        R2 rb;
        ra.x = ra.y = ra.z = ra.w = R(0);
        rb.x = rb.y = R(0);
        V3<R> T = mk<R>(R(1), R(1), R(1)), L = mk<R>(R(0), R(0), R(0));
        if (NC > 0 || GEN || DIR)
            tg.new_path();
        const int first_rr = a.min_bounces > 1 ? a.min_bounces : 1;
        for (;;) {
            // ---- lanes without a path take the wave's next samples -- once enough of them wait (the whole wave walks
            // through the camera code), or as many as still run
            const uint64_t idle_mask = wave_ballot(!live);
            const uint32_t n_idle = (uint32_t)__popcll(idle_mask), n_run = DRT_WAVE - n_idle;
            if (n_next < n_items && (n_idle >= a.regen_min || n_idle >= n_run)) {
                const uint32_t n = n_next + __builtin_amdgcn_mbcnt_hi((uint32_t)(idle_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle_mask, 0u));
                if (!live && n < n_items) {
                    pix = wbase + (n & (DRT_WAVE - 1));
                    const uint32_t gp = s_pgpix[pix];
                    if (gp != 0xFFFFFFFFu) {
                        pgpix = gp;
                        CameraLane<R> pc;
                        pc.cs0 = s_pcs[pix];
                        pc.ct0 = s_pct[pix];
                        key = path_camera<R>(a, pc, gp, pl.s_begin + (n >> 6), ra, rb);
                        kk = 0;
                        live = a.depth_cap > 0 && !(a.min_bounces <= 0 && rng_draw(a.rng_stream, key, 2) < a.rr_threshold);
                        T = mk<R>(R(1), R(1), R(1));
                        L = mk<R>(R(0), R(0), R(0));
                        if (NC > 0 || GEN || DIR)
                            tg.new_path();
                    }
                }
                n_next += n_idle < n_items - n_next ? n_idle : n_items - n_next;
            }
            const uint32_t n_live = (uint32_t)__popcll(wave_ballot(live));
            if (n_live == 0) {
                if (n_next >= n_items)
                    break;                                // the wave is through its samples
                continue;                                 // (all fresh paths were absorbed at depth 0, or belong to no pixel)
            }
            n_seg += n_live;
            // ---- one bounce, every lane at its own depth
            const bool rr_here = kk >= a.min_bounces;
            const R pk = rr_here ? pk_rr : R(1);                              // pathtracer.hpp:130
            const R inv_pk = rr_here ? inv_p_rr : R(1);
            const int rr_draws = kk - first_rr + 1;                           // roulette draws at depths 1 .. kk (draw_offset)
            const uint32_t n_theta = 2u * (uint32_t)kk + (uint32_t)(rr_draws > 0 ? rr_draws : 0) + camera_draw_base(a.min_bounces);
            const bool next_rr = (kk + 1) >= a.min_bounces;
            const bool next_cap = (kk + 1) >= a.depth_cap;
            bool alive, capped, on_light;
            uint32_t light;
            // the seed of the path's pixel (render.cpp:80: all ones; else the caller's image): read where a path meets a light
            V3<R> gp3 = mk<R>(R(1), R(1), R(1));
            const float* seed_px = (NP != 0 && adjoint) ? adjoint + (size_t)pgpix * 3 : (const float*)nullptr;
            path_bounce<R, SPEC, NP, NC, SG>(a, lds, tl, sc, params, recs, key, pk, inv_pk, n_theta, next_rr, next_cap, live, gp3,
                                                    ra, rb, T, L, tg, alive, capped, on_light, light, nullptr, false, seed_px, s_ih);
            if (!a.cap_is_roulette)
                n_capped += (uint32_t)__popcll(wave_ballot(capped));
            // ---- paths that ended here hand their radiance to their pixel
            const bool ended = live && !alive;
            if (wave_any(ended)) {
                if (ended) {
                    if (on_light) {
                        if (seed_px)
                            gp3 = mk<R>((R)seed_px[0], (R)seed_px[1], (R)seed_px[2]);
                        add_emission<R, NP, NC, LOSS>(lds, tl, params, light, inv_pk, T, gp3, L, tg
#ifdef DRT_SAMPLE_LOSS
                                                      , loss_q
#endif
                                                      );
                    }
#ifdef DRT_SAMPLE_LOSS
                    if (LOSS && seed_px) {
                        // the lane's path ends here, L is final (L = 0 where it reached no light): its value, against its pixel's target
                        R value_ = R(0);
                        V3<R> seed_ = mk<R>(R(0), R(0), R(0));
                        sample_loss<R>(loss_q, L, mk<R>((R)seed_px[0], (R)seed_px[1], (R)seed_px[2]), value_, seed_);
                        loss_sum += (double)value_;
                    }
#endif
                    if (L.x != R(0) || L.y != R(0) || L.z != R(0)) {
                        atomicAdd(&s_film[0][pix], (double)L.x);
                        atomicAdd(&s_film[REGEN ? 1 : 0][pix], (double)L.y);
                        atomicAdd(&s_film[REGEN ? 2 : 0][pix], (double)L.z);
                    }
                    if constexpr (REGEN && DIR) {
                        if (tg.dL.x != R(0) || tg.dL.y != R(0) || tg.dL.z != R(0)) {
                            atomicAdd(&s_tfilm[0][pix], (double)tg.dL.x);
                            atomicAdd(&s_tfilm[1][pix], (double)tg.dL.y);
                            atomicAdd(&s_tfilm[2][pix], (double)tg.dL.z);
                        }
                    }
                }
            }
            live = alive;
            ++kk;
        }
    }
    if (REGEN) {
        __syncthreads();                                  // (every wave's adds have landed)
        fx = s_film[0][threadIdx.x]; fy = s_film[REGEN ? 1 : 0][threadIdx.x]; fz = s_film[REGEN ? 2 : 0][threadIdx.x];
        if constexpr (REGEN && DIR) {
            tx = s_tfilm[0][threadIdx.x]; ty = s_tfilm[1][threadIdx.x]; tz = s_tfilm[2][threadIdx.x];
        }
    }

    if constexpr (SETS) {                                 // the plain image's sums: the last set (the context's own parameters)
        fx = tk[NC - 1][0]; fy = tk[NC - 1][1]; fz = tk[NC - 1][2];
    }
    if (pl.range < a.n_ranges) {
        if (fpart && pl.have) {
            double* f = fpart + ((size_t)pl.range * 3) * a.Pb + pl.lp;       // [range][channel][pixel]: coalesced
            f[0] = fx; f[(size_t)a.Pb] = fy; f[(size_t)a.Pb * 2] = fz;
        }
        if constexpr (GEN && NC == 1) if (gimg_part && pl.have) {
            // gradient image, general form: the lane's own adds to the row of the image's parameter
            double* f = gimg_part + ((size_t)pl.range * 3) * a.Pb + pl.lp;
            f[0] = (double)tg.gsum.x; f[(size_t)a.Pb] = (double)tg.gsum.y; f[(size_t)a.Pb * 2] = (double)tg.gsum.z;
        }
        if constexpr ((DIRS && !CROSS) || SETS || ALONG) if (gimg_part && pl.have) {
            // K directions / K sets: the pixel's sums in the Jacobian form's layout, [range][3 k + ch][pixel], for those the caller gave; with a
            // direction per set, 6 rows a set: [range][6 k + ch][pixel] the radiance sums, [range][6 k + 3 + ch][pixel] the derivative sums
            const uint32_t nd = a.dirs_out() < (uint32_t)NC ? a.dirs_out() : (uint32_t)NC;
            double* f = gimg_part + ((size_t)pl.range * (size_t)(nd * (3u * TK))) * a.Pb + pl.lp;
#pragma unroll
            for (int k = 0; k < TK * NC; ++k)
                if ((uint32_t)(k / TK) < nd) {
                    f[(size_t)(k * 3) * a.Pb] = tk[k][0]; f[(size_t)(k * 3 + 1) * a.Pb] = tk[k][1]; f[(size_t)(k * 3 + 2) * a.Pb] = tk[k][2];
                }
        }
        if constexpr (CROSS) if (gimg_part && pl.have) {
            // K directions with cross moments: [range][row][pixel] with 6 nd + 3 rows -- 3 nd derivative sums, 3 nd of Q, 3 of S2 --, for the
            // directions the caller gave
            const uint32_t nd = a.dirs_out() < (uint32_t)NC ? a.dirs_out() : (uint32_t)NC;
            double* f = gimg_part + ((size_t)pl.range * (size_t)(nd * 6u + 3u)) * a.Pb + pl.lp;
            double* fq = f + (size_t)(nd * 3u) * a.Pb;
#pragma unroll
            for (int k = 0; k < NC; ++k)
                if ((uint32_t)k < nd) {
                    f[(size_t)(k * 3) * a.Pb] = tk[k][0]; f[(size_t)(k * 3 + 1) * a.Pb] = tk[k][1]; f[(size_t)(k * 3 + 2) * a.Pb] = tk[k][2];
                    fq[(size_t)(k * 3) * a.Pb] = tg.Q[k][0]; fq[(size_t)(k * 3 + 1) * a.Pb] = tg.Q[k][1]; fq[(size_t)(k * 3 + 2) * a.Pb] = tg.Q[k][2];
                }
            double* fs = f + (size_t)(nd * 6u) * a.Pb;
            fs[0] = tg.S2[0]; fs[(size_t)a.Pb] = tg.S2[1]; fs[(size_t)a.Pb * 2] = tg.S2[2];
        }
        if constexpr (DIR && !DIRS) if (gimg_part && pl.have) {
            // forward mode: the pixel's derivative sums leave where a gradient image's do -- same layout, same finishing kernels
            double* f = gimg_part + ((size_t)pl.range * 3) * a.Pb + pl.lp;
            f[0] = tx; f[(size_t)a.Pb] = ty; f[(size_t)a.Pb * 2] = tz;
        }
        if constexpr (JAC) if (gimg_part && pl.have) {
            // the Jacobian: all rows of the lane's column -- the pixel's gradient sums of every parameter over the samples of this range,
            // [range][row][pixel] with the scene's own 3 x n_params rows (k_normal_eq reads them back, coalesced like the radiance partials)
            const int rows = (lds.sc.n_params < NP ? lds.sc.n_params : NP) * 3;
            double* f = gimg_part + ((size_t)pl.range * (size_t)rows) * a.Pb + pl.lp;
#pragma unroll
            for (int r = 0; r < NP * 3; ++r)
                if (r < rows)
                    f[(size_t)r * a.Pb] = (double)tg.acc[r * DRT_BLOCK];
        }
        if constexpr (NP > 0 && !JAC) if (gimg_part && pl.have) {
            // gradient image (README.md:142-145): a lane IS a pixel, its gradient sum of one parameter over the samples of
            // this range is that pixel's share -- same layout as the radiance partials, same finishing kernels
            const V3<R> v = tg.acc_get(a.gimg_param > 0 && a.gimg_param < NP ? a.gimg_param : 0);
            double* f = gimg_part + ((size_t)pl.range * 3) * a.Pb + pl.lp;
            f[0] = (double)v.x; f[(size_t)a.Pb] = (double)v.y; f[(size_t)a.Pb * 2] = (double)v.z;
        }
        store_counts(a, pl, counts, n_seg, n_capped);
#ifdef DRT_SAMPLE_LOSS
        if (LOSS && loss_part) {
            // the wave's sum, lanes added in a fixed order (every lane of the wave is here: `range` is the wave's)
            double v = loss_sum;
            for (int o2 = DRT_WAVE / 2; o2 > 0; o2 >>= 1)
                v += __shfl_down(v, o2);
            if (pl.lane == 0)
                loss_part[pl.w] = v;
        }
#endif
    }
    if constexpr (GEN || SGRAD)
        gen_finish(s_gen, a, gpart);
    else
    if constexpr (NP > 0 && !JAC) {
        double (*red)[DRT_FAST_PARAMS * 3] = s_red;
        if (REGEN) {
            __syncthreads();                               // (every thread has read its pixel's sums out of s_film)
            red = reinterpret_cast<double (*)[DRT_FAST_PARAMS * 3]>(&s_film[0][0]);
        }
        const int wv = threadIdx.x / DRT_WAVE;
#pragma unroll
        for (int r = 0; r < NP * 3; ++r) {
            double v = (double)tg.acc[r * DRT_BLOCK];
#pragma unroll
            for (int o2 = DRT_WAVE / 2; o2 > 0; o2 >>= 1)
                v += __shfl_down(v, o2);
            if (pl.lane == 0)
                red[wv][r] = v;
        }
        __syncthreads();
        if (threadIdx.x < DRT_FAST_PARAMS * 3) {
            double v = 0;
            if ((int)threadIdx.x < NP * 3)
                for (int ww = 0; ww < DRT_BLOCK / DRT_WAVE; ++ww)
                    v += red[ww][threadIdx.x];
            gpart[(size_t)blockIdx.x * (DRT_FAST_PARAMS * 3) + threadIdx.x] = v;
        }
    }
}

// ---- k_path_sets_cross: one path under K parameter sets, with every set's second moments (drt_hip_render_param_sets_cross) ------------
// The lockstep half of k_path for NP = DRT_NP_SETS, as an entry point of its own -- so that no instantiation of k_path changes its name
// or its code --: the same staging (stage_path_scene, path_tables_begin / stage_sets), the same camera, path_bounce and add_emission on
// the same operands in the same order, so set k's radiance sums keep the bits drt_hip_render_param_sets gives.  Beside them, per lane and
// after each sample, from the sample's own tg.L[k]:
//     S2_k[ch] += L_k[ch]^2          in fp64 (exact products for f32 operands)
// the raw moment an unbiased square of a pixel's residual needs (a U-statistic over the pixel's n samples): the mean over s != s' of
// (L_{k,s} - target)(L_{k,s'} - target) = r_k^2 - var(L_k) / n with the sample variance (S2_k - n m_k^2) / (n - 1).  Raw moments add across
// sample ranges.  At the end of its range a lane writes gpix[range][row][pixel] with 6 nd rows: 3 nd radiance sums (row 3 k + ch), then
// 3 nd of S2 (row 3 nd + 3 k + ch), nd = PathArgs::dirs_out(), the caller's sets; k_sets_cross_finish (below) forms the corrections per
// pixel.  Nothing goes to `fpart` (this call has no plain image) or `gpart`.
// blocks per CU (= waves per SIMD) of the f32 forms: the most that stay free of scratch (the compiler's report: DESIGN.md 9b)
#ifndef DRT_SETS_CROSS2_MIN_BLOCKS
#define DRT_SETS_CROSS2_MIN_BLOCKS 6      // (diffuse; the glossy forms keep 32-48 bytes of scratch at six: five)
#endif
#ifndef DRT_SETS_CROSS4_MIN_BLOCKS
#define DRT_SETS_CROSS4_MIN_BLOCKS 3      // (24-28 bytes of scratch at four)
#endif
#ifndef DRT_SETS_CROSS8_MIN_BLOCKS
#define DRT_SETS_CROSS8_MIN_BLOCKS 2
#endif
template <size_t RB, bool SPEC, int K>
constexpr int sets_cross_min_blocks()
{
    return RB == 4 ? (K <= 2 ? (SPEC ? 5 : DRT_SETS_CROSS2_MIN_BLOCKS) : (K <= 4 ? DRT_SETS_CROSS4_MIN_BLOCKS : DRT_SETS_CROSS8_MIN_BLOCKS))
                   : (K <= 2 ? 2 : 1);
}
template <typename R, bool SPEC, int K, typename SG>
__global__ void __launch_bounds__(DRT_BLOCK, (sets_cross_min_blocks<sizeof(R), SPEC, K>()))
k_path_sets_cross(PathArgs a, const DevScene<R>* __restrict__ sc, const R* __restrict__ params, const float* __restrict__ adjoint,
                  double* __restrict__ gpart, double* __restrict__ fpart, uint32_t* __restrict__ counts,
                  unsigned long long* __restrict__ total, double* __restrict__ gimg_part)
{
    static_assert(K == 2 || K == 4 || K == 8, "k_path_sets_cross: 2, 4 or 8 sets");
    (void)adjoint; (void)gpart; (void)fpart;              // (the path kernels share one argument list and one launch site)
    zero_totals(total);
    typedef typename Q4<R>::T R4;
    typedef typename Q2<R>::T R2;
    __shared__ PathSceneLds<R> lds;
    __shared__ TangentLds<R> s_tl;                        // (never staged: path_bounce's argument, unread in this form)
    stage_path_scene(lds, sc, params);
    const TangentLds<R>& tl = s_tl;

    const PathLane pl = path_lane(a);

    Tangents<R, DRT_NP_SETS, K> tg;
    path_tables_begin(tg, lds, params);
    double tk[K][3], s2[K][3];                            // per set: the radiance sums and the sums of squares of this lane's pixel over the range
#pragma unroll
    for (int k = 0; k < K; ++k) {
        tk[k][0] = tk[k][1] = tk[k][2] = 0.0;
        s2[k][0] = s2[k][1] = s2[k][2] = 0.0;
    }
    uint32_t n_seg = 0, n_capped = 0;                     // wave-uniform counters

    uint32_t gpix = 0, px = 0, py = 0;
    const V3<R> g = mk<R>(R(1), R(1), R(1));                    // render.cpp:80: radiance.backward(Vec3(1))
    if (pl.have) {
        gpix = path_global_pixel(a, a.p0 + pl.lp);
        py = gpix / (uint32_t)a.W;
        px = gpix - py * (uint32_t)a.W;
    }
    const CameraLane<R> cl = camera_lane<R>(a, px, py);
    constexpr bool ARGS_F32 = path_args_f32<R, SG>();
    const R pk_rr = ARGS_F32 ? (R)a.p_rr_f : (R)a.p_rr, inv_p_rr = ARGS_F32 ? (R)a.inv_p_rr_f : (R)a.inv_p_rr;
    ProgRecs<SG::n, R> recs;
    __shared__ typename PickT<(SG::n == 0), ProgLds, NoLds>::T s_prog;
    recs.lds = reinterpret_cast<const ProgLds*>(&s_prog);
    if (SG::n > 0)
        recs.template load<SG>(sc);
    if constexpr (sizeof(R) == 4 && SG::n == 0) {
        const DevScene<float>* scf = reinterpret_cast<const DevScene<float>*>(sc);
        if (threadIdx.x < DRT_PROG_SORTED_MAX) {
            s_prog.rec[threadIdx.x] = *reinterpret_cast<const float4*>(scf->sorted[threadIdx.x]);
            s_prog.shape[threadIdx.x] = scf->sorted_shape[threadIdx.x];
        }
        if (threadIdx.x < 8)
            s_prog.kind_begin[threadIdx.x] = scf->kind_begin[threadIdx.x];
        __syncthreads();
    }

    if (pl.range >= a.n_ranges)
        return;
    for (uint32_t sl = pl.s_begin; sl < pl.s_end; ++sl) {
        R4 ra;
        R2 rb;
        const uint32_t key = path_camera<R, ARGS_F32>(a, cl, gpix, px, py, sl, ra, rb);
        // pathtracer.hpp:128 at depth 0
        bool live = pl.have && a.depth_cap > 0 && !(a.min_bounces <= 0 && rng_draw(a.rng_stream, key, 2) < a.rr_threshold);
        V3<R> T = mk<R>(R(1), R(1), R(1)), L = mk<R>(R(0), R(0), R(0));
        uint32_t end_ids = DRT_ID_NONE;                   // emission parameter of the light the path ended on
        R end_inv_pk = R(1);
        tg.new_path();
        for (int kk = 0; kk < a.depth_cap; ++kk) {
            const uint32_t n_live = (uint32_t)__popcll(wave_ballot(live));
            if (n_live == 0)
                break;
            n_seg += n_live;
            const R pk = kk >= a.min_bounces ? pk_rr : R(1);                  // pathtracer.hpp:130
            const R inv_pk = kk >= a.min_bounces ? inv_p_rr : R(1);
            const uint32_t n_theta = draw_offset(kk, 0, a.min_bounces) + camera_draw_base(a.min_bounces);
            const bool next_rr = (kk + 1) >= a.min_bounces;
            const bool next_cap = (kk + 1) >= a.depth_cap;
            bool alive, capped, on_light;
            uint32_t light;
            path_bounce<R, SPEC, DRT_NP_SETS, K, SG, (DRT_FREEZE_BY_ROW != 0 && sizeof(R) == 4 && !SPEC && SG::n <= DRT_LEAN_MAX_SHAPES)>(a, lds, tl, sc, params, recs, key, pk, inv_pk, n_theta, next_rr, next_cap, live, g,
                                                    ra, rb, T, L, tg, alive, capped, on_light, light, nullptr, next_cap);
            // (a light without a BxDF ends the path; its emission is added once per sample, behind the loop)
            end_ids = on_light ? light : end_ids;
            end_inv_pk = on_light ? inv_pk : end_inv_pk;
            if (next_cap && !a.cap_is_roulette)
                n_capped += (uint32_t)__popcll(wave_ballot(capped));
            live = alive;
        }
        if (wave_any(end_ids != DRT_ID_NONE)) {
            if (end_ids != DRT_ID_NONE)
                add_emission<R, DRT_NP_SETS, K, false, PathSceneLds<R>, 0>(lds, tl, params, end_ids, end_inv_pk, T, g, L, tg);
        }
        // the sample's sums and squares, from its own values
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double lx = (double)tg.L[k].x, ly = (double)tg.L[k].y, lz = (double)tg.L[k].z;
            tk[k][0] += lx; tk[k][1] += ly; tk[k][2] += lz;
            s2[k][0] += lx * lx; s2[k][1] += ly * ly; s2[k][2] += lz * lz;
        }
    }
    if (gimg_part && pl.have) {
        // [range][row][pixel] with 6 nd rows -- 3 nd radiance sums, 3 nd of S2 --, for the sets the caller gave
        const uint32_t nd = a.dirs_out() < (uint32_t)K ? a.dirs_out() : (uint32_t)K;
        double* f = gimg_part + ((size_t)pl.range * (size_t)(nd * 6u)) * a.Pb + pl.lp;
        double* fs = f + (size_t)(nd * 3u) * a.Pb;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if ((uint32_t)k < nd) {
                store_rows3(f + (size_t)(k * 3) * a.Pb, a.Pb, tk[k][0], tk[k][1], tk[k][2]);
                store_rows3(fs + (size_t)(k * 3) * a.Pb, a.Pb, s2[k][0], s2[k][1], s2[k][2]);
            }
    }
    store_counts(a, pl, counts, n_seg, n_capped);
}

// ---- k_path_lean: the lockstep f32 column-form k_path with two more facts compiled in --------------------------------------
// What the host knows before it launches (shard_plan: PathForm::fixed, ::no_lit_bxdf), as it knows the slots' roles:
//   FIXED        the render has no roulette inside the loop: absorb == 1 at min_bounces == the depth cap (a.cap_is_roulette &&
//                a.min_bounces == a.depth_cap: the reference's -b depth -p 1, every configuration of the benchmark).  p_k = 1 / p_k = 1 at
//                every vertex, no vertex draws for the roulette, no path is "capped", and the draws of vertex k are 2 k + 2, 2 k + 3.
//   NO_LIT_BXDF  no shape of the scene has both a material and an emitter (the reference's scene; every scene whose lights have no BxDF):
//                the only emission of a path is the light it ends on.
// The kernel is k_path<R, false, NP, NCR, SG, false, false> with those constants in place -- x * 1.0f is exact, a term never added is
// never added: the same operations on the same operands in the same order, every sum keeps its bits -- as an entry point of its own, so
// that no instantiation of k_path changes its name or its code.  Forms: the gradient columns of <= 4 parameters (NP = 4) and forward
// only (NP = 0); no gradient image, no Jacobian, no loss seed: those renders keep k_path.
// The last vertex of a path, where the program is compiled in (SG::n > 0; the kind-sorted program keeps the loop as it was):
//   LIGHTS  the scene's pure lights as a bit set in scene order (shard_plan: PathForm::lights; 0: not known) -- the last vertex asks only
//           whether the path ended on one of them (path_bounce: LIGHTS);
//   and it stands behind the bounce loop, not inside it: with both hits in one loop body the compiler merged their common beginnings and
//   the plain bounce grew by 7 vector instructions (profiles/r17_path_ends.txt: 2.8 % SLOWER than without LIGHTS).
template <typename R, int NP, int NCR, typename SG, unsigned long long LIGHTS = 0ull>
__global__ void __launch_bounds__(DRT_BLOCK, (SG::n <= DRT_LEAN_MAX_SHAPES ? DRT_LEAN_PATH_MIN_BLOCKS : DRT_LOCKSTEP_GEN_MIN_BLOCKS))
k_path_lean(PathArgs a, const DevScene<R>* __restrict__ sc, const R* __restrict__ params, const float* __restrict__ adjoint,
            double* __restrict__ gpart, double* __restrict__ fpart, uint32_t* __restrict__ counts,
            unsigned long long* __restrict__ total, double* __restrict__ gimg_part)
{
    static_assert(sizeof(R) == 4 && (NP == 0 || NP == 4), "k_path_lean: f32, four parameters in columns or none");
    static_assert(!DRT_JACOBIAN_OF(NCR), "k_path_lean has no Jacobian form");
    static_assert(LIGHTS == 0ull || SG::n > 0, "k_path_lean: the light set belongs to a compiled-in program");
    (void)gimg_part;                                      // (the path kernels share one argument list and one launch site)
    zero_totals(total);
    typedef typename Q4<R>::T R4;
    typedef typename Q2<R>::T R2;
    constexpr int NC = DRT_NC_OF(NCR), ROLES = DRT_ROLES_OF(NCR);
    __shared__ PathSceneLds<R> lds;
    __shared__ double s_red[DRT_BLOCK / DRT_WAVE][DRT_FAST_PARAMS * 3];
    __shared__ TangentLds<R> s_tl;
    stage_path_scene(lds, sc, params);
    const TangentLds<R>& tl = s_tl;
    // the bounce's own tables (LeanLds): the hit shape's record and the colour's row, one address each
    constexpr bool BY_ROW = DRT_FREEZE_BY_ROW != 0 && SG::n <= DRT_LEAN_MAX_SHAPES;
    constexpr bool LEAN_REC = lean_rec<SG, NC, BY_ROW, true, true, false, R>();
    __shared__ typename PickT<LEAN_REC, LeanLds<SG::n, NC>, NoLds>::T s_lean;
    const LeanLds<SG::n, NC>* ll = reinterpret_cast<const LeanLds<SG::n, NC>*>(&s_lean);
    if (NC > 0)
        stage_tangents(s_tl, lds);
    if constexpr (LEAN_REC)
        stage_lean(s_lean, lds, s_tl);

    const PathLane pl = path_lane(a);

    Tangents<R, NP, NC> tg;
    __shared__ R s_acc[NP > 0 ? NP * 3 : 1][DRT_BLOCK];
    tg.acc = &s_acc[0][threadIdx.x];
#pragma unroll
    for (int p = 0; p < NP; ++p)
        tg.acc_set(p, mk<R>(R(0), R(0), R(0)));
    double fx = 0, fy = 0, fz = 0;                        // radiance sum of this lane's pixel over the range
    uint32_t n_seg = 0;                                   // wave-uniform counter

    uint32_t gpix = 0, px = 0, py = 0;
    V3<R> g = mk<R>(R(1), R(1), R(1));                    // render.cpp:80: radiance.backward(Vec3(1))
    if (pl.have) {
        gpix = path_global_pixel(a, a.p0 + pl.lp);
        py = gpix / (uint32_t)a.W;
        px = gpix - py * (uint32_t)a.W;
        if (NP != 0 && adjoint)
            g = mk<R>((R)adjoint[(size_t)gpix * 3], (R)adjoint[(size_t)gpix * 3 + 1], (R)adjoint[(size_t)gpix * 3 + 2]);
    }
    const CameraLane<R> cl = camera_lane<R>(a, px, py);
    constexpr bool ARGS_F32 = path_args_f32<R, SG>();
    ProgRecs<SG::n, R> recs;
    __shared__ typename PickT<(SG::n == 0), ProgLds, NoLds>::T s_prog;
    recs.lds = reinterpret_cast<const ProgLds*>(&s_prog);
    if (SG::n > 0)
        recs.template load<SG>(sc);
    if constexpr (SG::n == 0) {
        const DevScene<float>* scf = reinterpret_cast<const DevScene<float>*>(sc);
        if (threadIdx.x < DRT_PROG_SORTED_MAX) {
            s_prog.rec[threadIdx.x] = *reinterpret_cast<const float4*>(scf->sorted[threadIdx.x]);
            s_prog.shape[threadIdx.x] = scf->sorted_shape[threadIdx.x];
        }
        if (threadIdx.x < 8)
            s_prog.kind_begin[threadIdx.x] = scf->kind_begin[threadIdx.x];
        __syncthreads();
    }

    if (pl.range < a.n_ranges) {
        for (uint32_t sl = pl.s_begin; sl < pl.s_end; ++sl) {
            R4 ra;
            R2 rb;
            // (FOLD: the sample's key folded once, here; the camera's draws and the bounces' take the folded key -- drt_fold.h, path_bounce: FOLDED)
            constexpr bool FOLD = DRT_LEAN_FOLD_DRAWS != 0 && SG::n > 0;
            uint32_t kf = 0u, key;
            if constexpr (FOLD)
                key = path_camera_folded<ARGS_F32>(a, cl, gpix, sl, ra, rb, kf);
            else
                key = path_camera<R, ARGS_F32>(a, cl, gpix, px, py, sl, ra, rb);
            bool live = pl.have;                             // (pathtracer.hpp:128 at depth 0: min_bounces = the cap > 0, no roulette there either)
            V3<R> T = mk<R>(R(1), R(1), R(1)), L = mk<R>(R(0), R(0), R(0));
            uint32_t end_ids = DRT_ID_NONE;               // emission parameter of the light the path ended on
            if (NC > 0)
                tg.new_path();
            if constexpr (SG::n > 0 && DRT_LEAN_PEEL_LAST != 0) {
                // the last vertex behind the loop: the loop's body is the plain bounce -- no test for the last vertex, no code of it for the
                // compiler to merge with the bounce's.  `is_last`: known where the vertex stands in the code
                // LIVE_MASK: "this lane's path goes on" crosses the loop's back edge as the wave's mask in a scalar pair -- the bounce moves it on
                // by a scalar AND (path_bounce: live_mask) and a lane reads its bit back; carried as a bool it came round as 0 / 1 in a vector
                // register, v_cndmask + v_cmp at the top of every vertex.  The gradient form only: the forward-only kernel, two instructions
                // shorter per vertex with it all the same, ran 1.7 % SLOWER than without (profiles/r18_bounce_fusions.txt)
                constexpr bool LIVE_MASK = DRT_LEAN_LIVE_MASK != 0 && LEAN_REC && NP > 0;
                // MASK_REST (path_bounce): the bounce itself moves end_ids on where it carries the mask, and the segment count is added where it
                // stands -- left to sink behind the bounce, it too keeps the mask of `live` in a scalar pair across the masked block
                constexpr bool MASK_REST = LEAN_REC && lean_part(DRT_LEAN_MASK_REST, NP), END_IN_BOUNCE = MASK_REST && LIVE_MASK;
                uint64_t lm = LIVE_MASK ? wave_ballot(live) : 0ull;
                const auto vertex = [&](int kk, auto is_last) {
                    const uint32_t n_theta = 2u * (uint32_t)kk + 2u;   // draw_offset + camera_draw_base below min_bounces
                    constexpr bool next_cap = decltype(is_last)::value;
                    bool alive, capped, on_light;
                    uint32_t light;
                    if constexpr (LIVE_MASK)
                        live = __builtin_amdgcn_inverse_ballot_w64(lm);
                    path_bounce<R, false, NP, NC, SG, BY_ROW, true, true, LIGHTS>(
                        a, lds, tl, sc, params, recs, key, R(1), R(1), n_theta, false, next_cap, live, g, ra, rb, T, L, tg, alive, capped, on_light, light, nullptr, next_cap,
                        nullptr, nullptr, ll, LIVE_MASK ? &lm : nullptr, kf, END_IN_BOUNCE && !next_cap ? &end_ids : nullptr);
                    if (!(END_IN_BOUNCE && !next_cap))
                        end_ids = on_light ? light : end_ids;
                    live = alive;
                };
                const auto n_alive = [&]() { return (uint32_t)__popcll(LIVE_MASK ? lm : wave_ballot(live)); };
                for (int kk = 0; kk < a.depth_cap - 1; ++kk) {
                    const uint32_t n_live = n_alive();
                    if (n_live == 0)
                        break;
                    n_seg += n_live;
                    if constexpr (MASK_REST)
                        asm volatile("" : "+s"(n_seg));
                    vertex(kk, BoolT<false>());
                }
                const uint32_t n_live = n_alive();
                if (a.depth_cap > 0 && n_live != 0) {
                    n_seg += n_live;
                    vertex(a.depth_cap - 1, BoolT<true>());
                }
            } else
            for (int kk = 0; kk < a.depth_cap; ++kk) {
                const uint32_t n_live = (uint32_t)__popcll(wave_ballot(live));
                if (n_live == 0)
                    break;
                n_seg += n_live;
                const uint32_t n_theta = 2u * (uint32_t)kk + 2u;       // draw_offset + camera_draw_base below min_bounces
                const bool next_cap = (kk + 1) >= a.depth_cap;
                bool alive, capped, on_light;
                uint32_t light;
                path_bounce<R, false, NP, NC, SG, BY_ROW, true, true, LIGHTS>(
                    a, lds, tl, sc, params, recs, key, R(1), R(1), n_theta, false, next_cap, live, g, ra, rb, T, L, tg, alive, capped, on_light, light, nullptr, next_cap,
                    nullptr, nullptr, ll, nullptr, kf);
                end_ids = on_light ? light : end_ids;     // (its emission: once per sample, below)
                live = alive;
            }
            if (wave_any(end_ids != DRT_ID_NONE)) {
                if (end_ids != DRT_ID_NONE)
                    add_emission<R, NP, NC, false, PathSceneLds<R>, ROLES>(lds, tl, params, end_ids, R(1), T, g, L, tg);
            }
            fx += (double)L.x; fy += (double)L.y; fz += (double)L.z;
        }
        if (fpart && pl.have) {
            store_rows3(fpart + ((size_t)pl.range * 3) * a.Pb + pl.lp, a.Pb, fx, fy, fz);
        }
        store_counts(a, pl, counts, n_seg, 0u);                        // (no path is cut short by a cap that is the roulette's)
    }
    if constexpr (NP > 0)
        block_grad_sums<NP>(tg.acc, s_red, gpart, pl.lane);
}

// ---- k_path_views: one scene from several cameras in one launch (drt_hip_render_views) ------------------------------------------------
// The lockstep half of k_path for the forward-only form, the gradient columns and the general form, as an entry point of its own -- so that
// no instantiation of k_path changes its name or its code.  The grid is the single-frame grid once per view: `view_blocks` blocks a view,
// each view's waves exactly the waves drt_hip_render launches for that frame alone (the same spr, n_ranges and n_groups in `a0`), every view
// starting on a block boundary, so a block's gradient sums add the same four waves.  A block derives its view from its index and takes the
// view's camera constants, seed and stream from views[view] -- a wave-uniform address: scalar loads into scalar registers, where the
// kernel's arguments would have been -- into its own copy of the arguments; everything downstream (camera_lane, path_camera, path_bounce,
// add_emission) then runs as in k_path, on the same operands in the same order: view v's sums keep the bits of the single call.
// The partial sums gain the view as their outermost dimension: fpart[view][range][row][pixel], counts[view][row][wave of the view],
// gpart[block of the grid][row] (a view's blocks are consecutive), the general form's global history columns over the threads of the whole
// grid (a0.hist_stride); the adjoint images stand one behind the other.  k_views_finish (below) reduces them.
// (a closest-hit program type under a name of the shell's own: the same members, other instantiations of what takes it)
template <typename SG> struct ViewsSig : SG {};
struct PathView {
    double eye[3], fwd[3], right[3], up[3];
    double tan_half, aspect;
    float eye_f[3], fwd_f[3], right_f[3], up_f[3], cs_step_f, ct_step_f;   // cast on the host as path_batch casts PathArgs' own
    uint32_t seed, rng_stream;
};
// blocks per CU (= waves per SIMD): the budget of the lockstep k_path instantiation the form mirrors (path_min_blocks) -- but for the diffuse f64
// gradient forms, columns of four and general: at DRT_F64_MIN_BLOCKS the compiler reports 20-28 bytes of scratch per lane for the shell, as
// it does for those k_path instantiations themselves; with a block fewer the shell has none
template <size_t RB, bool SPEC, int NP, int NSG, int NCR>
constexpr int views_min_blocks()
{
    return (RB == 8 && !SPEC && NP != 0 && NP <= 4) ? DRT_F64_MIN_BLOCKS - 1 : path_min_blocks<RB, SPEC, NP, NSG, false, NCR>();
}
template <typename R, bool SPEC, int NP, int NCR, typename SG>
__global__ void __launch_bounds__(DRT_BLOCK, (views_min_blocks<sizeof(R), SPEC, NP, SG::n, NCR>()))
k_path_views(PathArgs a0, const PathView* __restrict__ views, uint32_t view_blocks, const DevScene<R>* __restrict__ sc, const R* __restrict__ params,
             const float* __restrict__ adjoint, double* __restrict__ gpart, double* __restrict__ fpart, uint32_t* __restrict__ counts,
             unsigned long long* __restrict__ total)
{
    static_assert(NP == 0 || NP == 4 || NP == 8 || NP == DRT_NP_ANY, "k_path_views: forward only, the gradient columns or the general form");
    static_assert(!DRT_JACOBIAN_OF(NCR) && DRT_ROLES_OF(NCR) == 0, "k_path_views has no Jacobian form and no roles");
    zero_totals(total);
    typedef typename Q4<R>::T R4;
    typedef typename Q2<R>::T R2;
    constexpr int NC = DRT_NC_OF(NCR);
    constexpr bool GEN = NP == DRT_NP_ANY;
    static_assert(!GEN || NC == 0, "k_path_views: the general form without a gradient image");
    // the block's view and its place among the view's blocks; the arguments as the single call's kernel would have had them
    const uint32_t view = __builtin_amdgcn_readfirstlane(blockIdx.x / view_blocks);
    const uint32_t view_block = blockIdx.x - view * view_blocks;
    PathArgs a = a0;
    {
        const PathView& v = views[view];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            a.eye[i] = v.eye[i]; a.fwd[i] = v.fwd[i]; a.right[i] = v.right[i]; a.up[i] = v.up[i];
            a.eye_f[i] = v.eye_f[i]; a.fwd_f[i] = v.fwd_f[i]; a.right_f[i] = v.right_f[i]; a.up_f[i] = v.up_f[i];
        }
        a.tan_half = v.tan_half; a.aspect = v.aspect;
        a.cs_step_f = v.cs_step_f; a.ct_step_f = v.ct_step_f;
        a.seed = v.seed; a.rng_stream = v.rng_stream;
    }
    const size_t view_waves = (size_t)a.n_groups * a.n_ranges;
    if (adjoint)
        adjoint += (size_t)view * (size_t)a.W * (size_t)a.H * 3;
    if (fpart)
        fpart += (size_t)view * ((size_t)a.n_ranges * 3 * a.Pb);
    counts += (size_t)view * (2 * view_waves);

    __shared__ PathSceneLds<R> lds;
    __shared__ double s_red[DRT_BLOCK / DRT_WAVE][DRT_FAST_PARAMS * 3];
    __shared__ TangentLds<R> s_tl;
    __shared__ typename PickT<GEN, GenBlock<R>, NoLds>::T s_gen;
    extern __shared__ uint32_t s_hist[];                  // GEN: [a.hist_lds][DRT_BLOCK] history words
    if constexpr (GEN)
        gen_zero(s_gen);
    stage_path_scene(lds, sc, params);
    const TangentLds<R>& tl = s_tl;
    if (NC > 0 && !GEN)
        stage_tangents(s_tl, lds);

    const PathLane pl = path_lane_in_frame(a, __builtin_amdgcn_readfirstlane(view_block * (DRT_BLOCK / DRT_WAVE) + threadIdx.x / DRT_WAVE));

    Tangents<R, NP, NC> tg;
    __shared__ R s_acc[NP > 0 ? NP * 3 : 1][DRT_BLOCK];
    tg.acc = &s_acc[0][threadIdx.x];
    if constexpr (GEN)
        gen_begin(s_gen, lds, sc, a, s_hist, reinterpret_cast<uint32_t*>(a.hist_ovf), tg);
    else {
#pragma unroll
        for (int p = 0; p < NP; ++p)
            tg.acc_set(p, mk<R>(R(0), R(0), R(0)));
    }
    double fx = 0, fy = 0, fz = 0;                        // radiance sum of this lane's pixel over the range
    uint32_t n_seg = 0, n_capped = 0;                     // wave-uniform counters

    uint32_t gpix = 0, px = 0, py = 0;                    // (the pixel within the view: the RNG key is the single call's)
    V3<R> g = mk<R>(R(1), R(1), R(1));                    // render.cpp:80: radiance.backward(Vec3(1))
    if (pl.have) {
        gpix = path_global_pixel(a, a.p0 + pl.lp);
        py = gpix / (uint32_t)a.W;
        px = gpix - py * (uint32_t)a.W;
        if (NP != 0 && adjoint)
            g = mk<R>((R)adjoint[(size_t)gpix * 3], (R)adjoint[(size_t)gpix * 3 + 1], (R)adjoint[(size_t)gpix * 3 + 2]);
    }
    const CameraLane<R> cl = camera_lane<R>(a, px, py);
    constexpr bool ARGS_F32 = path_args_f32<R, SG>();
    const R pk_rr = ARGS_F32 ? (R)a.p_rr_f : (R)a.p_rr, inv_p_rr = ARGS_F32 ? (R)a.inv_p_rr_f : (R)a.inv_p_rr;
    ProgRecs<SG::n, R> recs;
    __shared__ typename PickT<(SG::n == 0), ProgLds, NoLds>::T s_prog;
    recs.lds = reinterpret_cast<const ProgLds*>(&s_prog);
    if (SG::n > 0)
        recs.template load<SG>(sc);
    if constexpr (sizeof(R) == 4 && SG::n == 0) {
        const DevScene<float>* scf = reinterpret_cast<const DevScene<float>*>(sc);
        if (threadIdx.x < DRT_PROG_SORTED_MAX) {
            s_prog.rec[threadIdx.x] = *reinterpret_cast<const float4*>(scf->sorted[threadIdx.x]);
            s_prog.shape[threadIdx.x] = scf->sorted_shape[threadIdx.x];
        }
        if (threadIdx.x < 8)
            s_prog.kind_begin[threadIdx.x] = scf->kind_begin[threadIdx.x];
        __syncthreads();
    }

    if (pl.range < a.n_ranges) {
        for (uint32_t sl = pl.s_begin; sl < pl.s_end; ++sl) {
            R4 ra;
            R2 rb;
            const uint32_t key = path_camera<R, ARGS_F32>(a, cl, gpix, px, py, sl, ra, rb);
            // pathtracer.hpp:128 at depth 0
            bool live = pl.have && a.depth_cap > 0 && !(a.min_bounces <= 0 && rng_draw(a.rng_stream, key, 2) < a.rr_threshold);
            V3<R> T = mk<R>(R(1), R(1), R(1)), L = mk<R>(R(0), R(0), R(0));
            uint32_t end_ids = DRT_ID_NONE;               // emission parameter of the light the path ended on
            R end_inv_pk = R(1);
            if (NC > 0 || GEN)
                tg.new_path();
            for (int kk = 0; kk < a.depth_cap; ++kk) {
                const uint32_t n_live = (uint32_t)__popcll(wave_ballot(live));
                if (n_live == 0)
                    break;
                n_seg += n_live;
                const R pk = kk >= a.min_bounces ? pk_rr : R(1);                  // pathtracer.hpp:130
                const R inv_pk = kk >= a.min_bounces ? inv_p_rr : R(1);
                const uint32_t n_theta = draw_offset(kk, 0, a.min_bounces) + camera_draw_base(a.min_bounces);
                const bool next_rr = (kk + 1) >= a.min_bounces;
                const bool next_cap = (kk + 1) >= a.depth_cap;
                bool alive, capped, on_light;
                uint32_t light;
                // (the program's type under the shell's own name -- ViewsSig --: the bounce is then the shell's own instantiation.  Shared with
                //  k_path's, the forward-only f32 k_path's bounce had a second caller, which moved that kernel's inlining, a register and its stream)
                path_bounce<R, SPEC, NP, NC, ViewsSig<SG>, (DRT_FREEZE_BY_ROW != 0 && sizeof(R) == 4 && !SPEC && SG::n <= DRT_LEAN_MAX_SHAPES)>(a, lds, tl, sc, params, recs, key, pk, inv_pk, n_theta, next_rr, next_cap, live, g,
                                                        ra, rb, T, L, tg, alive, capped, on_light, light, nullptr, next_cap);
                // (a light without a BxDF ends the path; its emission is added once per sample, behind the loop)
                end_ids = on_light ? light : end_ids;
                end_inv_pk = on_light ? inv_pk : end_inv_pk;
                if (next_cap && !a.cap_is_roulette)
                    n_capped += (uint32_t)__popcll(wave_ballot(capped));
                live = alive;
            }
            if (wave_any(end_ids != DRT_ID_NONE)) {
                if (end_ids != DRT_ID_NONE)
                    add_emission<R, NP, NC, false, PathSceneLds<R>, 0>(lds, tl, params, end_ids, end_inv_pk, T, g, L, tg);
            }
            fx += (double)L.x; fy += (double)L.y; fz += (double)L.z;
        }
        if (fpart && pl.have)
            store_rows3(fpart + ((size_t)pl.range * 3) * a.Pb + pl.lp, a.Pb, fx, fy, fz);
        store_counts(a, pl, counts, n_seg, n_capped);
    }
    if constexpr (GEN)
        gen_finish(s_gen, a, gpart);
    else if constexpr (NP > 0)
        block_grad_sums<NP>(tg.acc, s_red, gpart, pl.lane);
}

// ---- k_path_pixels: a caller's batch of pixels from several cameras in one launch (drt_hip_render_pixels) -----------------------------
// k_path_views with one indirection: a lane's pixel is the caller's, pixels[the view's first entry + the lane's place in the view's list].
// View v's list is a "frame" of n_entries pixels -- n_groups = ceil(n_entries / 64) waves a sample range, every view on a block boundary, a
// view without entries without blocks -- and the sample ranges are the ones the plan picks for a SINGLE W x H x spp frame (a0.spr,
// a0.n_ranges), not re-tuned to the list's length: a lane then adds the samples the single call's lane of that pixel and range adds, in its
// order, and the finishing kernel adds the ranges the single call's finishing launch adds -- that is what makes an entry's radiance the
// single call's bits.  The RNG key of a sample is pixel spp + sample, so a pixel rendered alone draws what it draws inside its frame.
// A block finds its view by a scalar search over the at most 64 first blocks at the head of the table (a view without blocks shares its
// first block with its successor: the LAST view whose first block is not beyond the block's index is the one), takes the view's record
// through that wave-uniform index -- scalar loads -- and patches its copy of the arguments: camera, seed, stream, Pb = n_entries, n_groups.
// Partial sums: fpart per view [range][row][entry], counts per view [row][wave of the view], gpart[block of the grid][row], the general
// form's global history columns over the threads of the whole grid.  k_pixels_finish (below) reduces them.
template <typename SG> struct PixelsSig : SG {};
struct PixelView {
    PathView cam;
    uint32_t first_block, n_blocks, first_entry, n_entries, n_groups, pad;
    unsigned long long fpart_at, counts_at;               // doubles / words in front of the view's sums
};
struct PixelsHead {
    uint32_t first_block[64];                             // per view (DRT_HIP_MAX_VIEWS); behind it, 16-byte aligned: PixelView[n_views]
};
__host__ __device__ inline const PixelView* pixel_views(const PixelsHead* head) { return reinterpret_cast<const PixelView*>(head + 1); }
template <typename R, bool SPEC, int NP, int NCR, typename SG>
__global__ void __launch_bounds__(DRT_BLOCK, (views_min_blocks<sizeof(R), SPEC, NP, SG::n, NCR>()))
k_path_pixels(PathArgs a0, const PixelsHead* __restrict__ head, uint32_t n_views, const uint32_t* __restrict__ pixels, const DevScene<R>* __restrict__ sc,
              const R* __restrict__ params, const float* __restrict__ adjoint, double* __restrict__ gpart, double* __restrict__ fpart,
              uint32_t* __restrict__ counts, unsigned long long* __restrict__ total)
{
    static_assert(NP == 0 || NP == 4 || NP == 8 || NP == DRT_NP_ANY, "k_path_pixels: forward only, the gradient columns or the general form");
    static_assert(!DRT_JACOBIAN_OF(NCR) && DRT_ROLES_OF(NCR) == 0, "k_path_pixels has no Jacobian form and no roles");
    zero_totals(total);
    typedef typename Q4<R>::T R4;
    typedef typename Q2<R>::T R2;
    constexpr int NC = DRT_NC_OF(NCR);
    constexpr bool GEN = NP == DRT_NP_ANY;
    static_assert(!GEN || NC == 0, "k_path_pixels: the general form without a gradient image");
    // the block's view and its place among the view's blocks; the arguments as a single call's kernel over the list would have had them
    uint32_t view = 0;
    for (uint32_t i = 1; i < n_views; ++i)
        view = head->first_block[i] <= blockIdx.x ? i : view;
    view = __builtin_amdgcn_readfirstlane(view);
    PathArgs a = a0;
    uint32_t view_block, first_entry;
    {
        const PixelView& pv = pixel_views(head)[view];
        const PathView& v = pv.cam;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            a.eye[i] = v.eye[i]; a.fwd[i] = v.fwd[i]; a.right[i] = v.right[i]; a.up[i] = v.up[i];
            a.eye_f[i] = v.eye_f[i]; a.fwd_f[i] = v.fwd_f[i]; a.right_f[i] = v.right_f[i]; a.up_f[i] = v.up_f[i];
        }
        a.tan_half = v.tan_half; a.aspect = v.aspect;
        a.cs_step_f = v.cs_step_f; a.ct_step_f = v.ct_step_f;
        a.seed = v.seed; a.rng_stream = v.rng_stream;
        a.Pb = pv.n_entries; a.n_groups = pv.n_groups; a.p0 = 0;
        view_block = blockIdx.x - pv.first_block;
        first_entry = pv.first_entry;
        if (fpart)
            fpart += pv.fpart_at;
        counts += pv.counts_at;
    }
    pixels += first_entry;
    if (adjoint)
        adjoint += (size_t)first_entry * 3;

    __shared__ PathSceneLds<R> lds;
    __shared__ double s_red[DRT_BLOCK / DRT_WAVE][DRT_FAST_PARAMS * 3];
    __shared__ TangentLds<R> s_tl;
    __shared__ typename PickT<GEN, GenBlock<R>, NoLds>::T s_gen;
    extern __shared__ uint32_t s_hist[];                  // GEN: [a.hist_lds][DRT_BLOCK] history words
    if constexpr (GEN)
        gen_zero(s_gen);
    stage_path_scene(lds, sc, params);
    const TangentLds<R>& tl = s_tl;
    if (NC > 0 && !GEN)
        stage_tangents(s_tl, lds);

    const PathLane pl = path_lane_in_frame(a, __builtin_amdgcn_readfirstlane(view_block * (DRT_BLOCK / DRT_WAVE) + threadIdx.x / DRT_WAVE));

    Tangents<R, NP, NC> tg;
    __shared__ R s_acc[NP > 0 ? NP * 3 : 1][DRT_BLOCK];
    tg.acc = &s_acc[0][threadIdx.x];
    if constexpr (GEN)
        gen_begin(s_gen, lds, sc, a, s_hist, reinterpret_cast<uint32_t*>(a.hist_ovf), tg);
    else {
#pragma unroll
        for (int p = 0; p < NP; ++p)
            tg.acc_set(p, mk<R>(R(0), R(0), R(0)));
    }
    double fx = 0, fy = 0, fz = 0;                        // radiance sum of this lane's entry over the range
    uint32_t n_seg = 0, n_capped = 0;                     // wave-uniform counters

    uint32_t gpix = 0, px = 0, py = 0;                    // (the pixel within its frame: the RNG key is the single call's)
    V3<R> g = mk<R>(R(1), R(1), R(1));                    // render.cpp:80: radiance.backward(Vec3(1))
    if (pl.have) {
        gpix = pixels[pl.lp];                             // the one new line of the prologue: lane -> the caller's pixel
        py = gpix / (uint32_t)a.W;
        px = gpix - py * (uint32_t)a.W;
        if (NP != 0 && adjoint)
            g = mk<R>((R)adjoint[(size_t)pl.lp * 3], (R)adjoint[(size_t)pl.lp * 3 + 1], (R)adjoint[(size_t)pl.lp * 3 + 2]);
    }
    const CameraLane<R> cl = camera_lane<R>(a, px, py);
    constexpr bool ARGS_F32 = path_args_f32<R, SG>();
    const R pk_rr = ARGS_F32 ? (R)a.p_rr_f : (R)a.p_rr, inv_p_rr = ARGS_F32 ? (R)a.inv_p_rr_f : (R)a.inv_p_rr;
    ProgRecs<SG::n, R> recs;
    __shared__ typename PickT<(SG::n == 0), ProgLds, NoLds>::T s_prog;
    recs.lds = reinterpret_cast<const ProgLds*>(&s_prog);
    if (SG::n > 0)
        recs.template load<SG>(sc);
    if constexpr (sizeof(R) == 4 && SG::n == 0) {
        const DevScene<float>* scf = reinterpret_cast<const DevScene<float>*>(sc);
        if (threadIdx.x < DRT_PROG_SORTED_MAX) {
            s_prog.rec[threadIdx.x] = *reinterpret_cast<const float4*>(scf->sorted[threadIdx.x]);
            s_prog.shape[threadIdx.x] = scf->sorted_shape[threadIdx.x];
        }
        if (threadIdx.x < 8)
            s_prog.kind_begin[threadIdx.x] = scf->kind_begin[threadIdx.x];
        __syncthreads();
    }

    if (pl.range < a.n_ranges) {
        for (uint32_t sl = pl.s_begin; sl < pl.s_end; ++sl) {
            R4 ra;
            R2 rb;
            const uint32_t key = path_camera<R, ARGS_F32>(a, cl, gpix, px, py, sl, ra, rb);
            // pathtracer.hpp:128 at depth 0
            bool live = pl.have && a.depth_cap > 0 && !(a.min_bounces <= 0 && rng_draw(a.rng_stream, key, 2) < a.rr_threshold);
            V3<R> T = mk<R>(R(1), R(1), R(1)), L = mk<R>(R(0), R(0), R(0));
            uint32_t end_ids = DRT_ID_NONE;               // emission parameter of the light the path ended on
            R end_inv_pk = R(1);
            if (NC > 0 || GEN)
                tg.new_path();
            for (int kk = 0; kk < a.depth_cap; ++kk) {
                const uint32_t n_live = (uint32_t)__popcll(wave_ballot(live));
                if (n_live == 0)
                    break;
                n_seg += n_live;
                const R pk = kk >= a.min_bounces ? pk_rr : R(1);                  // pathtracer.hpp:130
                const R inv_pk = kk >= a.min_bounces ? inv_p_rr : R(1);
                const uint32_t n_theta = draw_offset(kk, 0, a.min_bounces) + camera_draw_base(a.min_bounces);
                const bool next_rr = (kk + 1) >= a.min_bounces;
                const bool next_cap = (kk + 1) >= a.depth_cap;
                bool alive, capped, on_light;
                uint32_t light;
                // (the program's type under the shell's own name -- PixelsSig --: the bounce is the shell's own instantiation, and neither
                //  k_path's nor k_path_views' bounce gains a caller, which has moved a kernel's inlining before: HISTORY.md)
                path_bounce<R, SPEC, NP, NC, PixelsSig<SG>, (DRT_FREEZE_BY_ROW != 0 && sizeof(R) == 4 && !SPEC && SG::n <= DRT_LEAN_MAX_SHAPES)>(a, lds, tl, sc, params, recs, key, pk, inv_pk, n_theta, next_rr, next_cap, live, g,
                                                        ra, rb, T, L, tg, alive, capped, on_light, light, nullptr, next_cap);
                // (a light without a BxDF ends the path; its emission is added once per sample, behind the loop)
                end_ids = on_light ? light : end_ids;
                end_inv_pk = on_light ? inv_pk : end_inv_pk;
                if (next_cap && !a.cap_is_roulette)
                    n_capped += (uint32_t)__popcll(wave_ballot(capped));
                live = alive;
            }
            if (wave_any(end_ids != DRT_ID_NONE)) {
                if (end_ids != DRT_ID_NONE)
                    add_emission<R, NP, NC, false, PathSceneLds<R>, 0>(lds, tl, params, end_ids, end_inv_pk, T, g, L, tg);
            }
            fx += (double)L.x; fy += (double)L.y; fz += (double)L.z;
        }
        if (fpart && pl.have)
            store_rows3(fpart + ((size_t)pl.range * 3) * a.Pb + pl.lp, a.Pb, fx, fy, fz);
        store_counts(a, pl, counts, n_seg, n_capped);
    }
    if constexpr (GEN)
        gen_finish(s_gen, a, gpart);
    else if constexpr (NP > 0)
        block_grad_sums<NP>(tg.acc, s_red, gpart, pl.lane);
}

// ---- the unbiased integration operator (integrate.hpp:11-24, 39-52; README.md:104-136) in one launch ------------------
// The reference's IntegrateBackward does not reuse the forward samples: where a gradient arrives at a vertex it draws a
// FRESH direction, evaluates forward(sample) -- a whole new suffix path -- back-propagates grad / pdf through
// brdf * radiance * cos, and the recursion continues down the NEW path (O(depth^2) segments per camera sample).  Like
// k_path, a lane is a pixel and everything lives in registers:
//   forward walk from the eye (radiance -> the image; its first vertex starts the chain), then per chain vertex:
//   emission gradient, fresh direction, suffix walk (radiance L'), colour gradient += L' * g / pdf * cos * bs,
//   g *= f * cos / pdf, and the suffix's first vertex is the next chain vertex.
// All draws of a path come from ONE stream in the order the reference consumes them (a counter per lane): camera 2,
// then per vertex [roulette of its depth] theta phi -- including the roulette draw the reference spends AFTER a light
// without BxDF (its zero-direction continuation is traced "faithfully" before it misses; oracle/ref_harness.cpp).
// One walk = the bounce of k_path (path_bounce, forward-only) iterated while any lane of the wave still traces.
template <typename R, bool SPEC, typename SG>
__device__ inline void unbiased_walk(const PathArgs& a, const PathSceneLds<R>& lds, const TangentLds<R>& tl, const DevScene<R>* __restrict__ sc,
                                     const R* __restrict__ params, const ProgRecs<SG::n, R>& recs, uint32_t key,
                                     R pk_rr, R inv_p_rr, bool live, typename Q4<R>::T ra, typename Q2<R>::T rb, int kk,
                                     uint32_t& nd, uint32_t& n_seg, uint32_t& n_capped, V3<R>& L, PathVertex<R>& first, bool& any_vertex)
{
    V3<R> T = mk<R>(R(1), R(1), R(1));
    L = mk<R>(R(0), R(0), R(0));
    any_vertex = false;
    Tangents<R, 0, 0> none;
    const V3<R> g1 = mk<R>(R(1), R(1), R(1));
    for (;;) {
        const uint32_t n_live = (uint32_t)__popcll(wave_ballot(live));
        if (n_live == 0)
            break;
        n_seg += n_live;
        const bool rr_here = kk >= a.min_bounces;
        const R pk = rr_here ? pk_rr : R(1), inv_pk = rr_here ? inv_p_rr : R(1);
        const bool next_rr = (kk + 1) >= a.min_bounces, next_cap = (kk + 1) >= a.depth_cap;
        bool alive, capped, on_light;
        uint32_t light;
        PathVertex<R> v;
        path_bounce<R, SPEC, 0, 0, SG>(a, lds, tl, sc, params, recs, key, pk, inv_pk, nd, next_rr, next_cap, live, g1, ra, rb, T, L,
                                              none, alive, capped, on_light, light, &v);
        // the roulette of the next depth is drawn unless a user cap ends the path first (pathtracer.hpp:128 behind the cap test)
        const uint32_t rr_drawn = (next_rr && (!next_cap || a.cap_draws)) ? 1u : 0u;
        if (live) {
            if (!any_vertex && v.hit) {
                first = v;
                any_vertex = true;
            }
            nd += v.scattered ? 2u + rr_drawn : (v.hit ? rr_drawn : 0u);
        }
        if (wave_any(live && on_light)) {
            if (live && on_light)
                add_emission<R, 0, 0>(lds, tl, params, light, inv_pk, T, g1, L, none);
        }
        if (!a.cap_is_roulette)
            n_capped += (uint32_t)__popcll(wave_ballot(live && capped));
        live = alive;
        ++kk;
    }
}

#ifndef DRT_UNBIASED_MIN_BLOCKS
#define DRT_UNBIASED_MIN_BLOCKS 4    // blocks per CU the f32 k_path_unbiased is compiled for: 128 registers + 96 B of scratch per lane.  Left to itself the
                                     // compiler takes 153-173 registers (three / two waves per SIMD).  Config 3's frame, ms per launch, builds alternating:
                                     // diffuse 5.47 -> 4.77 at four (five: 4.93, six: 5.56), with the glossy sphere 9.41 -> 6.65 (7.09, 7.98)
#endif
template <typename R, bool SPEC, int NP, typename SG>
__global__ void __launch_bounds__(DRT_BLOCK, (sizeof(R) == 4 ? DRT_UNBIASED_MIN_BLOCKS : 1))
k_path_unbiased(PathArgs a, const DevScene<R>* __restrict__ sc, const R* __restrict__ params, const float* __restrict__ adjoint,
                double* __restrict__ gpart, double* __restrict__ fpart, uint32_t* __restrict__ counts,
                unsigned long long* __restrict__ total)
{
    zero_totals(total);
    typedef typename Q4<R>::T R4;
    typedef typename Q2<R>::T R2;
    __shared__ PathSceneLds<R> lds;
    __shared__ double s_red[DRT_BLOCK / DRT_WAVE][DRT_FAST_PARAMS * 3];
    // NP = DRT_NP_ANY: any number of parameters -- the chain's two adds per vertex (the light's colour, the BxDF's colour) go
    // to the wave's gradient table in LDS (Tangents<R, DRT_NP_ANY>; no vertex history: the chain IS the reverse sweep)
    constexpr bool GEN = NP == DRT_NP_ANY;
    __shared__ typename PickT<GEN, GenBlock<R>, NoLds>::T s_gen;
    if constexpr (GEN)
        gen_zero(s_gen);
    stage_path_scene(lds, sc, params);
    const TangentLds<R>& tl = *reinterpret_cast<const TangentLds<R>*>(&lds);   // (forward-only walks never touch it)
    Tangents<R, GEN ? DRT_NP_ANY : 0, 0> gt;
    if constexpr (GEN)
        gen_begin(s_gen, lds, sc, a, (uint32_t*)nullptr, (uint32_t*)nullptr, gt);

    const PathLane pl = path_lane(a);

    V3<R> acc[NP > 0 ? NP : 1];
#pragma unroll
    for (int p = 0; p < NP; ++p)
        acc[p] = mk<R>(R(0), R(0), R(0));
    double fx = 0, fy = 0, fz = 0;
    uint32_t n_seg = 0, n_capped = 0;
    uint32_t gpix = 0, px = 0, py = 0;
    V3<R> g0 = mk<R>(R(1), R(1), R(1));                    // render.cpp:80: radiance.backward(Vec3(1))
    if (pl.have) {
        gpix = path_global_pixel(a, a.p0 + pl.lp);
        py = gpix / (uint32_t)a.W;
        px = gpix - py * (uint32_t)a.W;
        if (adjoint)
            g0 = mk<R>((R)adjoint[(size_t)gpix * 3], (R)adjoint[(size_t)gpix * 3 + 1], (R)adjoint[(size_t)gpix * 3 + 2]);
    }
    const CameraLane<R> cl = camera_lane<R>(a, px, py);
    constexpr bool ARGS_F32 = path_args_f32<R, SG>();
    const R pk_rr = ARGS_F32 ? (R)a.p_rr_f : (R)a.p_rr, inv_p_rr = ARGS_F32 ? (R)a.inv_p_rr_f : (R)a.inv_p_rr;
    ProgRecs<SG::n, R> recs;
    __shared__ ProgLds s_prog;
    recs.lds = &s_prog;
    if (SG::n > 0)
        recs.template load<SG>(sc);
    if (sizeof(R) == 4 && SG::n == 0) {
        const DevScene<float>* scf = reinterpret_cast<const DevScene<float>*>(sc);
        if (threadIdx.x < DRT_PROG_SORTED_MAX) {
            s_prog.rec[threadIdx.x] = *reinterpret_cast<const float4*>(scf->sorted[threadIdx.x]);
            s_prog.shape[threadIdx.x] = scf->sorted_shape[threadIdx.x];
        }
        if (threadIdx.x < 8)
            s_prog.kind_begin[threadIdx.x] = scf->kind_begin[threadIdx.x];
        __syncthreads();
    }
    // is the roulette of depth d drawn at all?  (not behind a user cap: the reference tests the cap first)
    auto rr_drawn = [&](int d) { return d >= a.min_bounces && (d < a.depth_cap || a.cap_draws != 0); };

    if (pl.range < a.n_ranges) {
        for (uint32_t sl = pl.s_begin; sl < pl.s_end; ++sl) {
            R4 ra;
            R2 rb;
            const uint32_t key = path_camera<R, ARGS_F32>(a, cl, gpix, px, py, sl, ra, rb);
            uint32_t nd = 2;                                  // the camera's two draws
            bool live = pl.have && a.depth_cap > 0;
            if (rr_drawn(0)) {                                // pathtracer.hpp:128 at depth 0
                live = live && !(rng_draw(a.rng_stream, key, nd) < a.rr_threshold);
                ++nd;
            }
            V3<R> L0;
            PathVertex<R> cur;
            bool in_chain;
            unbiased_walk<R, SPEC, SG>(a, lds, tl, sc, params, recs, key, pk_rr, inv_p_rr, live, ra, rb, 0, nd, n_seg, n_capped, L0,
                                              cur, in_chain);
            fx += (double)L0.x; fy += (double)L0.y; fz += (double)L0.z;
            in_chain = in_chain && pl.have;
            int cdepth = 0;
            V3<R> g = g0;
            while (wave_any(in_chain)) {
                // ---- at the chain vertex: emission gradient, fresh direction (integrate.hpp:13-16)
                V3<R> gq = mk<R>(R(0), R(0), R(0)), fcol = gq;
                R bs = R(0);
                bool go = false;
                R4 sa = ra;
                R2 sb = rb;
                uint32_t cid = DRT_ID_NONE;
                if (in_chain) {
                    const R inv_pk = cdepth >= a.min_bounces ? inv_p_rr : R(1);
                    const V3<R> g1 = g * inv_pk;                  // "/ p" of trace()
                    const uint32_t eid = cur.ids >> 16;
                    cid = cur.ids & 0xFFFFu;
                    if constexpr (GEN) {
                        if (eid < DRT_PATH_LDS_PARAMS) {
                            const uint32_t row = pid_unpack(gt.gl->invc[eid][3]) & 0xFFFFu;
                            if (row != DRT_SLOT_NONE)
                                gt.add(row, g1);
                        }
                    }
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        const bool own = eid == (uint32_t)p;
                        acc[p] = mk<R>(acc[p].x + (own ? g1.x : R(0)), acc[p].y + (own ? g1.y : R(0)), acc[p].z + (own ? g1.z : R(0)));
                    }
                    if (cid == DRT_ID_NONE) {
                        in_chain = false;                         // no BxDF: f = 0, nothing below
                    } else {
                        const DevMaterial<R>& m = lds.sc.materials[cur.material];
                        V3<R> wo;
                        R q;
                        sample_bxdf<R, SPEC>(m, cur.nrm, cur.d, rng_draw(a.rng_stream, key, nd), rng_draw(a.rng_stream, key, nd + 1), wo, q, bs);
                        nd += 2;
                        const R c = dot(cur.nrm, wo);
                        gq = g1 * div_r(c, q);                    // grad / pdf (integrate.hpp:17), times cos
                        fcol = load_param<R, true>(lds, params, (int)cid) * bs;
                        go = (cdepth + 1) < a.depth_cap;
                        if (rr_drawn(cdepth + 1)) {
                            go = go && !(rng_draw(a.rng_stream, key, nd) < a.rr_threshold);
                            ++nd;
                        }
                        const V3<R> no = cur.P + wo * R(1e-3);
                        sa.x = no.x; sa.y = no.y; sa.z = no.z; sa.w = wo.x;
                        sb.x = wo.y; sb.y = wo.z;
                    }
                }
                // ---- forward(sample): the suffix from the fresh direction
                V3<R> Ls;
                PathVertex<R> nxt;
                bool any_vertex;
                unbiased_walk<R, SPEC, SG>(a, lds, tl, sc, params, recs, key, pk_rr, inv_p_rr, in_chain && go, sa, sb, cdepth + 1, nd,
                                                  n_seg, n_capped, Ls, nxt, any_vertex);
                // ---- gradients of this vertex; the chain moves on to the suffix's first vertex
                if (in_chain) {
                    const V3<R> df = Ls * gq * bs;                // MulBackward, brdf side
                    if constexpr (GEN) {
                        if (cid < DRT_PATH_LDS_PARAMS) {
                            const uint32_t row = pid_unpack(gt.gl->invc[cid][3]) & 0xFFFFu;
                            if (row != DRT_SLOT_NONE)
                                gt.add(row, df);
                        }
                    }
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        const bool own = cid == (uint32_t)p;
                        acc[p] = mk<R>(acc[p].x + (own ? df.x : R(0)), acc[p].y + (own ? df.y : R(0)), acc[p].z + (own ? df.z : R(0)));
                    }
                    if (!any_vertex) {
                        in_chain = false;                         // the suffix is a constant
                    } else {
                        g = fcol * gq;                            // MulBackward, radiance side
                        cur = nxt;
                        ++cdepth;
                    }
                }
            }
        }
        if (fpart && pl.have) {
            store_rows3(fpart + ((size_t)pl.range * 3) * a.Pb + pl.lp, a.Pb, fx, fy, fz);
        }
        store_counts(a, pl, counts, n_seg, n_capped);
    }
    if constexpr (GEN)
        gen_finish(s_gen, a, gpart);
    else
    {   // block_grad_sums' two stages, written out: the columns come from the lane's registers
        const int wv = threadIdx.x / DRT_WAVE;
#pragma unroll
        for (int r = 0; r < NP * 3; ++r) {
            const V3<R> v3 = acc[r / 3];
            double v = (double)(r % 3 == 0 ? v3.x : (r % 3 == 1 ? v3.y : v3.z));
#pragma unroll
            for (int o2 = DRT_WAVE / 2; o2 > 0; o2 >>= 1)
                v += __shfl_down(v, o2);
            if (pl.lane == 0)
                s_red[wv][r] = v;
        }
        __syncthreads();
        if (threadIdx.x < DRT_FAST_PARAMS * 3) {
            double v = 0;
            if ((int)threadIdx.x < NP * 3)
                for (int ww = 0; ww < DRT_BLOCK / DRT_WAVE; ++ww)
                    v += s_red[ww][threadIdx.x];
            gpart[(size_t)blockIdx.x * (DRT_FAST_PARAMS * 3) + threadIdx.x] = v;
        }
    }
}

// film[p0 + j] += sum over the sample ranges of one batch, in range order (deterministic)
__global__ void __launch_bounds__(DRT_BLOCK)
k_film_parts(const double* __restrict__ fpart, uint32_t n_ranges, uint32_t Pb, uint32_t p0, double* __restrict__ film)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < Pb; j += stride) {
        double r = 0, g = 0, b = 0;
        for (uint32_t q = 0; q < n_ranges; ++q) {
            const double* f = fpart + ((size_t)q * 3) * Pb + j;
            r += f[0]; g += f[(size_t)Pb]; b += f[(size_t)Pb * 2];
        }
        double* f = film + (size_t)(p0 + j) * 3;
        f[0] += r; f[1] += g; f[2] += b;
    }
}

// ---- everything behind a k_path launch that covers the whole frame, in ONE launch --------------------------------
// (a single-batch render otherwise enqueues three memsets and four small kernels: film sums, resolve, K7, segment
// totals -- 30 us of launches around a 15 us k_path on a 128 x 128 x 4 frame).  Same sums in the same order as
// k_film_parts + k_resolve, k_gradreduce and k_sum_counts, written instead of added to zeroed buffers: bitwise the same.
//   blocks [0, film_blocks):                  out[pixel] = float(sum over the sample ranges, in range order, / spp)
//   blocks [film_blocks, + grad_words):       grad[p] = sum over k_path's blocks of gpart[block][p], fixed order (p >= n_rows: 0)
//   the rest:                                 total[0] += segments, total[3] += capped paths (integers; k_path zeroed them)
__global__ void __launch_bounds__(DRT_BLOCK)
k_path_finish(PathArgs a, const double* __restrict__ fpart, float* __restrict__ out, uint32_t film_blocks,
              const double* __restrict__ gpart, int n_blocks, int n_rows, int row_stride, double* __restrict__ grad, uint32_t grad_words,
              const uint32_t* __restrict__ counts, uint32_t n_waves, unsigned long long* __restrict__ total, uint32_t count_rows = 2,
              const unsigned short* __restrict__ slot_map = nullptr)
{
    // (slot_map, the general form of the path kernels: gpart's rows are table rows, DevScene::grad_slot maps parameters to them)
    // (count_rows = 3, k_path_mesh: a third word per wave, the rays its BVH walk took -> total[5])
    __shared__ double red[DRT_BLOCK];
    if (blockIdx.x < film_blocks) {
        const uint32_t stride = film_blocks * DRT_BLOCK;
        const double inv = 1.0 / (double)a.spp;
        for (uint32_t j = blockIdx.x * DRT_BLOCK + threadIdx.x; j < a.Pb; j += stride) {
            double r = 0, g = 0, b = 0;
            for (uint32_t q = 0; q < a.n_ranges; ++q) {
                const double* f = fpart + ((size_t)q * 3) * a.Pb + j;
                r += f[0]; g += f[(size_t)a.Pb]; b += f[(size_t)a.Pb * 2];
            }
            const uint32_t gp = path_global_pixel(a, a.p0 + j);
            // (one 12-byte store per lane: `out` may be host memory -- asynchronous host-buffer renders write the image
            //  straight into the pinned block -- and whole lines travel better than three strided dwords)
            drt_f3 px;
            px.x = (float)(r * inv); px.y = (float)(g * inv); px.z = (float)(b * inv);
            *reinterpret_cast<drt_f3_u*>(out + (size_t)gp * 3) = px;
        }
        return;
    }
    if (blockIdx.x < film_blocks + grad_words) {
        const int p = (int)(blockIdx.x - film_blocks);
        int src = p;
        if (slot_map) {
            const int slot = slot_map[p / 3];
            src = slot == (int)DRT_SLOT_NONE ? n_rows : slot * 3 + p % 3;
        }
        double v = 0;
        if (src < n_rows)
            for (int b = threadIdx.x; b < n_blocks; b += DRT_BLOCK)
                v += gpart[(size_t)b * row_stride + src];
        red[threadIdx.x] = v;
        __syncthreads();
        for (int off = DRT_BLOCK / 2; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off)
                red[threadIdx.x] += red[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0)
            grad[p] = red[0];
        return;
    }
    {
        const uint32_t nb = gridDim.x - film_blocks - grad_words, me = blockIdx.x - film_blocks - grad_words;
        unsigned long long seg = 0, cap = 0, wlk = 0;
        for (uint32_t i = me * DRT_BLOCK + threadIdx.x; i < n_waves; i += nb * DRT_BLOCK) {
            seg += counts[i];
            cap += counts[(size_t)n_waves + i];
            if (count_rows > 2)
                wlk += counts[(size_t)n_waves * 2 + i];
        }
        for (int off = DRT_WAVE / 2; off > 0; off >>= 1) {
            seg += __shfl_down(seg, off);
            cap += __shfl_down(cap, off);
            wlk += __shfl_down(wlk, off);
        }
        if ((threadIdx.x & (DRT_WAVE - 1)) == 0) {
            if (seg) atomicAdd(total, seg);
            if (cap) atomicAdd(total + 3, cap);
            if (wlk) atomicAdd(total + 5, wlk);
        }
    }
}

// ---- the two stages of a frame-wide sum in fp64 behind the forms below: no atomics, every addition in a fixed order, so the same call
// gives the same bits
// first stage: the thread's NV running sums -> wave (shuffles) -> block (LDS); thread v < NV writes the block's sum of value v to
// part[at + v]  (base and offset apart, as the kernels wrote it: added up before the call the address costs them their instruction streams)
template <int NV>
__device__ inline void block_sums(const double (&acc)[NV], double* __restrict__ part, size_t at)
{
    __shared__ double red[DRT_BLOCK / DRT_WAVE][NV];
    const int wv = threadIdx.x / DRT_WAVE;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        double s = acc[v];
#pragma unroll
        for (int o2 = DRT_WAVE / 2; o2 > 0; o2 >>= 1)
            s += __shfl_down(s, o2);
        if ((threadIdx.x & (DRT_WAVE - 1)) == 0)
            red[wv][v] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = 0;
        for (int ww = 0; ww < DRT_BLOCK / DRT_WAVE; ++ww)
            s += red[ww][threadIdx.x];
        part[at + threadIdx.x] = s;
    }
}

// second stage: one value's partials over the first stage's n_blocks blocks, block b's from part_of(b) -- a strided sum per thread, then an
// LDS tree over the kernel's red[DRT_BLOCK]; the sum is red[0].  (The array and the index are the caller's: with an array of its own and
// the partials as pointer + stride, k_sets_along_sums and k_normal_eq_finish changed their register counts)
template <typename F>
__device__ inline void add_blocks(double* red, int n_blocks, F part_of)
{
    double s = 0;
    for (int b = threadIdx.x; b < n_blocks; b += DRT_BLOCK)
        s += part_of(b);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = DRT_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
}

// ---- the Gauss-Newton normal equations of a frame (drt_hip_render_normal_equations) -------------------------------------
// Behind a launch of k_path's Jacobian form: jpart[range][3 p + ch][pixel] holds, per pixel of the shard, the sums over one sample range of
// d radiance_ch / d c_{p,ch} (a radiance channel depends on the same channel of every parameter only: T_ch = prod c_{p_j,ch} m_j), fpart the
// radiance sums.  Per channel (blockIdx.y) and pixel, in fp64:
//     J_p = (sum over the ranges, in range order) / spp          0 where the parameter requires no gradient
//     r   = radiance mean - target   |   the caller's residual
//     A[p][q] += J_p J_q  (q >= p)      b[p] += J_p r      loss += r r          DRT_NEQ_VALUES(NP) running sums per thread
// then thread -> wave (shuffles) -> block (LDS) in a fixed order, one partial per block and channel; k_normal_eq_finish adds the blocks
// in a fixed order and mirrors A.  No atomics: the same call gives the same bits.  Memory-bound: 8 n_ranges (P + 1) bytes come in per
// pixel and channel, coalesced (VW = 2: two neighbouring pixels per lane, 16-byte loads; the host picks it where the batch's pixel count is even).
// The Jacobian images leave in the same pass where the caller wants them (float, the layout of P gradient images): n_out of them, the
// caller's parameters -- n_par, the rows of jpart, also counts the constant the scene appends for a mirror.
#define DRT_NEQ_VALUES(np) ((np) * ((np) + 1) / 2 + (np) + 1)
template <int NP, int VW>
__global__ void __launch_bounds__(DRT_BLOCK)
k_normal_eq(PathArgs a, const double* __restrict__ jpart, const double* __restrict__ fpart, int n_par, int n_out, uint32_t grad_mask,
            const float* __restrict__ target, const float* __restrict__ residual, float* __restrict__ out_jac, double* __restrict__ part)
{
    constexpr int NV = DRT_NEQ_VALUES(NP);
    typedef typename PickT<VW == 2, double2, double>::T DV;
    const int ch = (int)blockIdx.y;
    const size_t Pb = a.Pb, rows = (size_t)n_par * 3, npix = (size_t)a.W * (size_t)a.H;
    const double inv = 1.0 / (double)a.spp;
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k)
        acc[k] = 0.0;
    const uint32_t n_items = (a.Pb + VW - 1) / VW;
    for (uint32_t it = blockIdx.x * DRT_BLOCK + threadIdx.x; it < n_items; it += gridDim.x * DRT_BLOCK) {
        const uint32_t j = it * VW;
        double Js[NP][VW], Ls[VW];
#pragma unroll
        for (int v = 0; v < VW; ++v) {
            Ls[v] = 0.0;
#pragma unroll
            for (int p = 0; p < NP; ++p)
                Js[p][v] = 0.0;
        }
        for (uint32_t q = 0; q < a.n_ranges; ++q) {
            const double* fj = jpart + ((size_t)q * rows + (size_t)ch) * Pb + j;
            const DV lv = *reinterpret_cast<const DV*>(fpart + ((size_t)q * 3 + (size_t)ch) * Pb + j);
#pragma unroll
            for (int p = 0; p < NP; ++p)
                if (p < n_par) {
                    const DV jv = *reinterpret_cast<const DV*>(fj + (size_t)(p * 3) * Pb);
#pragma unroll
                    for (int v = 0; v < VW; ++v)
                        Js[p][v] += reinterpret_cast<const double*>(&jv)[v];
                }
#pragma unroll
            for (int v = 0; v < VW; ++v)
                Ls[v] += reinterpret_cast<const double*>(&lv)[v];
        }
#pragma unroll
        for (int v = 0; v < VW; ++v) {
            const size_t gp = path_global_pixel(a, a.p0 + j + (uint32_t)v);
            double J[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p)
                J[p] = ((grad_mask >> p) & 1u) ? Js[p][v] * inv : 0.0;
            const double r = target ? Ls[v] * inv - (double)target[gp * 3 + (size_t)ch] : (double)residual[gp * 3 + (size_t)ch];
            if (out_jac) {
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    if (p < n_out)             // (the caller's parameters: a mirror's internal constant behind them has a row in jpart, no image)
                        out_jac[((size_t)p * npix + gp) * 3 + (size_t)ch] = (float)J[p];
            }
            int k = 0;
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int q2 = p; q2 < NP; ++q2)
                    acc[k++] += J[p] * J[q2];
#pragma unroll
            for (int p = 0; p < NP; ++p)
                acc[k++] += J[p] * r;
            acc[k] += r * r;
        }
    }
    // (block_sums(), written out: through the function this kernel's resource report moves -- 96 -> 95 and 90 -> 88 SGPRs at width 4, 36 -> 39
    //  and 35 -> 37 SGPR spills at width 8 -- and a memory-bound kernel's time is not argued from a report)
    __shared__ double red[DRT_BLOCK / DRT_WAVE][NV];
    const int wv = threadIdx.x / DRT_WAVE;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o2 = DRT_WAVE / 2; o2 > 0; o2 >>= 1)
            v += __shfl_down(v, o2);
        if ((threadIdx.x & (DRT_WAVE - 1)) == 0)
            red[wv][k] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < NV) {
        double v = 0;
        for (int ww = 0; ww < DRT_BLOCK / DRT_WAVE; ++ww)
            v += red[ww][threadIdx.x];
        part[((size_t)ch * gridDim.x + blockIdx.x) * NV + threadIdx.x] = v;
    }
}

// ... its second stage: block (channel, value) adds that value's partials over k_normal_eq's blocks -- a strided sum per thread, then an LDS
// tree, both in a fixed order -- and writes it where it belongs: A[ch][p][q] and its mirror A[ch][q][p], b[ch][p], loss[ch], for the n_out
// parameters of the caller (np_w: the width k_normal_eq was instantiated for)
__global__ void __launch_bounds__(DRT_BLOCK)
k_normal_eq_finish(const double* __restrict__ part, int n_blocks, int np_w, int n_out, double* __restrict__ out_A, double* __restrict__ out_b,
                   double* __restrict__ out_loss)
{
    __shared__ double red[DRT_BLOCK];
    const int nv = DRT_NEQ_VALUES(np_w);
    const int ch = (int)blockIdx.x / nv, k = (int)blockIdx.x - ch * nv;
    add_blocks(red, n_blocks, [&](int b) { return part[((size_t)ch * n_blocks + b) * nv + k]; });
    if (threadIdx.x != 0)
        return;
    const int n_tri = np_w * (np_w + 1) / 2;
    if (k < n_tri) {
        int p = 0, first = 0;                                // row p of the upper triangle starts at `first` and holds np_w - p values
        while (k >= first + (np_w - p)) {
            first += np_w - p;
            ++p;
        }
        const int q = p + (k - first);
        if (p < n_out && q < n_out) {
            out_A[((size_t)ch * n_out + p) * n_out + q] = red[0];
            out_A[((size_t)ch * n_out + q) * n_out + p] = red[0];
        }
    } else if (k < n_tri + np_w) {
        if (k - n_tri < n_out)
            out_b[(size_t)ch * n_out + (k - n_tri)] = red[0];
    } else if (out_loss)
        out_loss[ch] = red[0];
}

// ---- the images and losses of a frame under K parameter sets (drt_hip_render_param_sets) -----------------------------------------
// Behind a launch of k_path's parameter-set form: spart[range][3 k + ch][pixel] holds, per pixel of the shard, set k's radiance sums over
// one sample range.  Per pixel and set, in fp64: the sum over the ranges in range order, the mean, the set's image (float and / or
// double, the layout of n_sets images) where the caller wants it, and with a target the residual mean - target, whose square goes into the
// thread's running sum of (set, channel) -- at most DRT_SETS_VALUES = 3 DRT_HIP_MAX_PARAM_SETS of them.  Then thread -> wave (shuffles) ->
// block (LDS) in a fixed order, one partial per block; k_sets_loss_finish adds the blocks in a fixed order.  No atomics: the same call
// gives the same bits.  k_normal_eq's structure and grid rule, a pixel per thread.
#define DRT_SETS_VALUES 24
__global__ void __launch_bounds__(DRT_BLOCK)
k_sets_finish(PathArgs a, const double* __restrict__ spart, int n_sets, const float* __restrict__ target, float* __restrict__ out_img,
              double* __restrict__ out_img64, double* __restrict__ part)
{
    const size_t Pb = a.Pb, rows = (size_t)n_sets * 3, npix = (size_t)a.W * (size_t)a.H;
    const double inv = 1.0 / (double)a.spp;
    double acc[DRT_SETS_VALUES];
#pragma unroll
    for (int v = 0; v < DRT_SETS_VALUES; ++v)
        acc[v] = 0.0;
    for (uint32_t j = blockIdx.x * DRT_BLOCK + threadIdx.x; j < a.Pb; j += gridDim.x * DRT_BLOCK) {
        const size_t gp = path_global_pixel(a, a.p0 + j);
        double tg[3] = {0.0, 0.0, 0.0};
        if (target) {
            tg[0] = (double)target[gp * 3]; tg[1] = (double)target[gp * 3 + 1]; tg[2] = (double)target[gp * 3 + 2];
        }
#pragma unroll
        for (int v = 0; v < DRT_SETS_VALUES; ++v)
            if (v < (int)rows) {
                double sum = 0.0;
                for (uint32_t q = 0; q < a.n_ranges; ++q)
                    sum += spart[((size_t)q * rows + (size_t)v) * Pb + j];
                const double mean = sum * inv;
                const size_t at = ((size_t)(v / 3) * npix + gp) * 3 + (size_t)(v % 3);
                if (out_img) out_img[at] = (float)mean;
                if (out_img64) out_img64[at] = mean;
                if (target) {
                    const double r = mean - tg[v % 3];
                    acc[v] += r * r;
                }
            }
    }
    if (!part)
        return;
    block_sums(acc, part, (size_t)blockIdx.x * DRT_SETS_VALUES);
}

// ... its second stage: block v adds value v's partials over k_sets_finish's blocks -- a strided sum per thread, then an LDS tree, both
// in a fixed order -- into out_loss[set][channel]
__global__ void __launch_bounds__(DRT_BLOCK)
k_sets_loss_finish(const double* __restrict__ part, int n_blocks, int n_values, double* __restrict__ out_loss)
{
    __shared__ double red[DRT_BLOCK];
    const int v = (int)blockIdx.x;
    add_blocks(red, n_blocks, [&](int b) { return part[(size_t)b * DRT_SETS_VALUES + v]; });
    if (threadIdx.x == 0 && v < n_values)
        out_loss[v] = red[0];
}

// ---- the images and the unbiased losses of a frame under K parameter sets (drt_hip_render_param_sets_cross) ------------------------
// Behind a launch of k_path_sets_cross: spart[range][row][pixel] holds, per pixel of the shard and sample range, set k's radiance sums
// (row 3 k + ch) and the sums of its samples' squares S2 (row 3 n_sets + 3 k + ch).  Per pixel, set and channel, in fp64, both sums over
// the ranges in range order, n = spp:
//     m = sum L / n      r = m - target      noise = (S2 - (sum L) m) / ((n - 1) n)      the sample variance of L over n (k_cross_eq's form)
//     loss[k][ch] += r r - noise      bias[k][ch] += noise
// the set's image (float, the layout of n_sets images: k_sets_finish's mean) and its variance image (noise, the same layout) where the
// caller wants them.  2 DRT_SETS_VALUES running sums per thread -- value 3 k + ch the loss, DRT_SETS_VALUES + 3 k + ch the bias --, then
// block_sums; k_sets_cross_sums adds the blocks in a fixed order.  No atomics: the same call gives the same bits.  k_sets_finish's
// structure and grid rule.
__global__ void __launch_bounds__(DRT_BLOCK)
k_sets_cross_finish(PathArgs a, const double* __restrict__ spart, int n_sets, const float* __restrict__ target, float* __restrict__ out_img,
                    float* __restrict__ out_var, double* __restrict__ part)
{
    const size_t Pb = a.Pb, half = (size_t)n_sets * 3, rows = half * 2, npix = (size_t)a.W * (size_t)a.H;
    const double n = (double)a.spp, inv = 1.0 / n, inv_pairs = 1.0 / ((n - 1.0) * n);
    double acc[2 * DRT_SETS_VALUES];
#pragma unroll
    for (int v = 0; v < 2 * DRT_SETS_VALUES; ++v)
        acc[v] = 0.0;
    for (uint32_t j = blockIdx.x * DRT_BLOCK + threadIdx.x; j < a.Pb; j += gridDim.x * DRT_BLOCK) {
        const size_t gp = path_global_pixel(a, a.p0 + j);
        const double tg[3] = {(double)target[gp * 3], (double)target[gp * 3 + 1], (double)target[gp * 3 + 2]};
#pragma unroll
        for (int v = 0; v < DRT_SETS_VALUES; ++v)
            if (v < (int)half) {
                double sum = 0.0, sq = 0.0;
                for (uint32_t q = 0; q < a.n_ranges; ++q) {
                    sum += spart[((size_t)q * rows + (size_t)v) * Pb + j];
                    sq += spart[((size_t)q * rows + half + (size_t)v) * Pb + j];
                }
                const double mean = sum * inv, r = mean - tg[v % 3];
                const double noise = (sq - sum * mean) * inv_pairs;
                const size_t at = ((size_t)(v / 3) * npix + gp) * 3 + (size_t)(v % 3);
                if (out_img) out_img[at] = (float)mean;
                if (out_var) out_var[at] = (float)noise;
                acc[v] += r * r - noise;
                acc[DRT_SETS_VALUES + v] += noise;
            }
    }
    block_sums(acc, part, (size_t)blockIdx.x * (2 * DRT_SETS_VALUES));
}

// ... its second stage: block v adds value v's partials over k_sets_cross_finish's blocks -- a strided sum per thread, then an LDS tree,
// both in a fixed order -- into out_loss[set][channel] or out_bias[set][channel] (where the caller gave it)
__global__ void __launch_bounds__(DRT_BLOCK)
k_sets_cross_sums(const double* __restrict__ part, int n_blocks, int n_values, double* __restrict__ out_loss, double* __restrict__ out_bias)
{
    __shared__ double red[DRT_BLOCK];
    const int v = (int)blockIdx.x % DRT_SETS_VALUES;
    double* out = (int)blockIdx.x < DRT_SETS_VALUES ? out_loss : out_bias;
    add_blocks(red, n_blocks, [&](int b) { return part[(size_t)b * (2 * DRT_SETS_VALUES) + blockIdx.x]; });
    if (threadIdx.x == 0 && v < n_values && out)
        out[v] = red[0];
}

// ---- the images, losses, slopes and curvatures of a frame under K parameter sets with a direction each (drt_hip_render_param_sets_along) ----
// Behind a launch of k_path's form of that name: spart[range][6 k + ch][pixel] holds, per pixel of the shard, set k's radiance sums over one
// sample range and spart[range][6 k + 3 + ch][pixel] the sums of its derivative along d_k.  Per pixel, set and channel, in fp64: both sums
// over the ranges in range order, the means m and t, the set's images (float and / or double, the layout of n_sets images) where the caller
// wants them, and three running sums of the thread -- r r and 2 r t with the residual r = m - target (where there is a target), and t t:
// the loss phi_k, its slope along d_k and the Gauss-Newton curvature |J d_k|^2 -- at most DRT_SETS_ALONG_VALUES = 9 DRT_HIP_MAX_SETS_ALONG of
// them, value (3 k + ch) * 3 + {0, 1, 2}.  Then thread -> wave (shuffles) -> block (LDS) in a fixed order, one partial per block;
// k_sets_along_sums adds the blocks in a fixed order.  No atomics: the same call gives the same bits.  k_sets_finish's structure and grid rule.
#define DRT_SETS_ALONG_VALUES 36
__global__ void __launch_bounds__(DRT_BLOCK)
k_sets_along_finish(PathArgs a, const double* __restrict__ spart, int n_sets, const float* __restrict__ target, float* __restrict__ out_img,
                    double* __restrict__ out_img64, float* __restrict__ out_tan, double* __restrict__ out_tan64, double* __restrict__ part)
{
    const size_t Pb = a.Pb, rows = (size_t)n_sets * 6, npix = (size_t)a.W * (size_t)a.H;
    const double inv = 1.0 / (double)a.spp;
    double acc[DRT_SETS_ALONG_VALUES];
#pragma unroll
    for (int v = 0; v < DRT_SETS_ALONG_VALUES; ++v)
        acc[v] = 0.0;
    for (uint32_t j = blockIdx.x * DRT_BLOCK + threadIdx.x; j < a.Pb; j += gridDim.x * DRT_BLOCK) {
        const size_t gp = path_global_pixel(a, a.p0 + j);
        double tg[3] = {0.0, 0.0, 0.0};
        if (target) {
            tg[0] = (double)target[gp * 3]; tg[1] = (double)target[gp * 3 + 1]; tg[2] = (double)target[gp * 3 + 2];
        }
#pragma unroll
        for (int v = 0; v < DRT_SETS_ALONG_VALUES / 3; ++v)          // v = 3 k + ch
            if (v < n_sets * 3) {
                const size_t row = (size_t)(v / 3) * 6 + (size_t)(v % 3);
                double sm = 0.0, st = 0.0;
                for (uint32_t q = 0; q < a.n_ranges; ++q) {
                    sm += spart[((size_t)q * rows + row) * Pb + j];
                    st += spart[((size_t)q * rows + row + 3) * Pb + j];
                }
                const double m = sm * inv, t = st * inv;
                const size_t at = ((size_t)(v / 3) * npix + gp) * 3 + (size_t)(v % 3);
                if (out_img) out_img[at] = (float)m;
                if (out_img64) out_img64[at] = m;
                if (out_tan) out_tan[at] = (float)t;
                if (out_tan64) out_tan64[at] = t;
                if (target) {
                    const double r = m - tg[v % 3];
                    acc[v * 3] += r * r;
                    acc[v * 3 + 1] += 2.0 * r * t;
                }
                acc[v * 3 + 2] += t * t;
            }
    }
    if (!part)
        return;
    block_sums(acc, part, (size_t)blockIdx.x * DRT_SETS_ALONG_VALUES);
}

// ... its second stage: block v adds value v's partials over k_sets_along_finish's blocks -- a strided sum per thread, then an LDS tree, both
// in a fixed order -- into out_loss / out_dloss / out_curv [set][channel], whichever the caller gave
__global__ void __launch_bounds__(DRT_BLOCK)
k_sets_along_sums(const double* __restrict__ part, int n_blocks, int n_values, double* __restrict__ out_loss, double* __restrict__ out_dloss,
                  double* __restrict__ out_curv)
{
    __shared__ double red[DRT_BLOCK];
    const int v = (int)blockIdx.x;
    add_blocks(red, n_blocks, [&](int b) { return part[(size_t)b * DRT_SETS_ALONG_VALUES + v]; });
    if (threadIdx.x == 0 && v < n_values) {
        double* out = v % 3 == 0 ? out_loss : (v % 3 == 1 ? out_dloss : out_curv);
        if (out)
            out[v / 3] = red[0];
    }
}

// ---- the summed gradients of a frame under K parameter sets (drt_hip_render_param_sets_grad) ---------------------------------------
// Behind a launch of k_path's form of that name: gpart[block][k R + row] holds the block's fp64 sums of set k's table rows (gen_finish), R =
// set_rows = 3 per parameter that requires a gradient.  Block (k, parameter, channel) adds its row over k_path's blocks -- a strided sum per
// thread, then an LDS tree, both in a fixed order -- into out[k][parameter][channel]; a parameter without a row (slot_map: DevScene::grad_slot)
// gets zero.  No atomics: the same call gives the same bits.
__global__ void __launch_bounds__(DRT_BLOCK)
k_sets_grad_finish(const double* __restrict__ gpart, int n_blocks, int row_stride, int set_rows, int n_out, const unsigned short* __restrict__ slot_map,
                   double* __restrict__ out)
{
    __shared__ double red[DRT_BLOCK];
    const int k = (int)blockIdx.x / (n_out * 3), pc = (int)blockIdx.x - k * (n_out * 3);
    const int slot = slot_map[pc / 3];
    const bool none = slot == (int)DRT_SLOT_NONE || slot * 3 >= set_rows;
    const int src = none ? 0 : k * set_rows + slot * 3 + pc % 3;
    add_blocks(red, none ? 0 : n_blocks, [&](int b) { return gpart[(size_t)b * row_stride + src]; });
    if (threadIdx.x == 0)
        out[blockIdx.x] = red[0];
}

// ---- everything behind a k_path_views launch, in ONE launch (drt_hip_render_views) ----------------------------------------------------
// k_path_finish over the views' partial sums, view v's with the sums and the order the single call's finishing launch has over that frame's:
//   blocks [0, n_views film_blocks):          out[v][pixel] = float(sum over the sample ranges, in range order, / spp), film_blocks a view
//   blocks [.., + grad_words):                word p of every view's gradient -- the sum over the VIEW's blocks of gpart[block][p], a strided sum
//                                             per thread, then an LDS tree, as k_path_finish adds a frame's -- to view_grads[v][p], and their
//                                             sum in view order, in fp64, to grad_sum[p].  A parameter that requires no gradient (slot_map:
//                                             DevScene::grad_slot) gets zero; general: gpart's rows are table rows, slot_map maps to them
//   the rest:                                 total[0] += segments, total[3] += capped paths over all views (integers; k_path_views zeroed them)
// No atomics on a float: the same call gives the same bits.
__global__ void __launch_bounds__(DRT_BLOCK)
k_views_finish(PathArgs a, uint32_t n_views, const double* __restrict__ fpart, float* __restrict__ out, uint32_t film_blocks,
               const double* __restrict__ gpart, int view_blocks, int n_rows, int row_stride, int general, const unsigned short* __restrict__ slot_map,
               double* __restrict__ view_grads, double* __restrict__ grad_sum, uint32_t grad_words,
               const uint32_t* __restrict__ counts, uint32_t view_waves, unsigned long long* __restrict__ total)
{
    __shared__ double red[DRT_BLOCK];
    const uint32_t all_film = n_views * film_blocks;
    if (blockIdx.x < all_film) {
        const uint32_t v = blockIdx.x / film_blocks, fb = blockIdx.x - v * film_blocks;
        const double* fv = fpart + (size_t)v * ((size_t)a.n_ranges * 3 * a.Pb);
        float* ov = out + (size_t)v * (size_t)a.W * (size_t)a.H * 3;
        const uint32_t stride = film_blocks * DRT_BLOCK;
        const double inv = 1.0 / (double)a.spp;
        for (uint32_t j = fb * DRT_BLOCK + threadIdx.x; j < a.Pb; j += stride) {
            double r = 0, g = 0, b = 0;
            for (uint32_t q = 0; q < a.n_ranges; ++q) {
                const double* f = fv + ((size_t)q * 3) * a.Pb + j;
                r += f[0]; g += f[(size_t)a.Pb]; b += f[(size_t)a.Pb * 2];
            }
            const uint32_t gp = path_global_pixel(a, a.p0 + j);
            drt_f3 px;
            px.x = (float)(r * inv); px.y = (float)(g * inv); px.z = (float)(b * inv);
            *reinterpret_cast<drt_f3_u*>(ov + (size_t)gp * 3) = px;
        }
        return;
    }
    if (blockIdx.x < all_film + grad_words) {
        const int p = (int)(blockIdx.x - all_film);
        const int slot = slot_map[p / 3];
        const int src = slot == (int)DRT_SLOT_NONE ? n_rows : (general ? slot * 3 + p % 3 : p);
        double sum = 0;
        for (uint32_t v = 0; v < n_views; ++v) {
            double x = 0;
            if (src < n_rows)
                for (int b = threadIdx.x; b < view_blocks; b += DRT_BLOCK)
                    x += gpart[((size_t)v * view_blocks + b) * row_stride + src];
            red[threadIdx.x] = x;
            __syncthreads();
            for (int off = DRT_BLOCK / 2; off > 0; off >>= 1) {
                if ((int)threadIdx.x < off)
                    red[threadIdx.x] += red[threadIdx.x + off];
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                if (view_grads)
                    view_grads[(size_t)v * grad_words + p] = red[0];
                sum = v == 0 ? red[0] : sum + red[0];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0 && grad_sum)
            grad_sum[p] = sum;
        return;
    }
    {
        const uint32_t first = all_film + grad_words, nb = gridDim.x - first, me = blockIdx.x - first;
        const uint64_t n = (uint64_t)n_views * view_waves;
        unsigned long long seg = 0, cap = 0;
        for (uint64_t i = (uint64_t)me * DRT_BLOCK + threadIdx.x; i < n; i += (uint64_t)nb * DRT_BLOCK) {
            const uint64_t v = i / view_waves, w = i - v * view_waves;
            const uint32_t* cv = counts + v * 2 * view_waves;
            seg += cv[w];
            cap += cv[(size_t)view_waves + w];
        }
        for (int off = DRT_WAVE / 2; off > 0; off >>= 1) {
            seg += __shfl_down(seg, off);
            cap += __shfl_down(cap, off);
        }
        if ((threadIdx.x & (DRT_WAVE - 1)) == 0) {
            if (seg) atomicAdd(total, seg);
            if (cap) atomicAdd(total + 3, cap);
        }
    }
}

// ---- everything behind a k_path_pixels launch, in ONE launch (drt_hip_render_pixels) --------------------------------------------------
// k_views_finish over lists in place of frames:
//   blocks [0, film_blocks):       out[entry] = float(sum over the sample ranges, in range order, in fp64, / spp) for the entries of all
//                                  views, in the caller's order (an entry's view: the last one whose first entry is not beyond it)
//   blocks [.., + grad_words):     word p of every view's gradient -- the sum over the VIEW's blocks of gpart[block][p] in k_views_finish's
//                                  order: strided per thread, then the LDS tree; a view without blocks gives zero -- to view_grads[v][p], and
//                                  their sum in view order, in fp64, to grad_sum[p]
//   the rest:                      total[0] += segments, total[3] += capped paths over all views (integers; k_path_pixels zeroed them)
// No atomics on a float: the same call gives the same bits.
__global__ void __launch_bounds__(DRT_BLOCK)
k_pixels_finish(PathArgs a, const PixelsHead* __restrict__ head, uint32_t n_views, uint32_t n_entries, const double* __restrict__ fpart,
                float* __restrict__ out, uint32_t film_blocks, const double* __restrict__ gpart, int n_rows, int row_stride, int general,
                const unsigned short* __restrict__ slot_map, double* __restrict__ view_grads, double* __restrict__ grad_sum, uint32_t grad_words,
                const uint32_t* __restrict__ counts, unsigned long long* __restrict__ total)
{
    __shared__ double red[DRT_BLOCK];
    const PixelView* views = pixel_views(head);
    if (blockIdx.x < film_blocks) {
        __shared__ uint32_t s_first[64];
        if (threadIdx.x < 64)
            s_first[threadIdx.x] = threadIdx.x < n_views ? views[threadIdx.x].first_entry : 0xFFFFFFFFu;
        __syncthreads();
        const double inv = 1.0 / (double)a.spp;
        for (uint32_t e = blockIdx.x * DRT_BLOCK + threadIdx.x; e < n_entries; e += film_blocks * DRT_BLOCK) {
            uint32_t v = 0;
            for (uint32_t i = 1; i < n_views; ++i)
                v = s_first[i] <= e ? i : v;
            const uint32_t Pb = views[v].n_entries, j = e - views[v].first_entry;
            const double* fv = fpart + views[v].fpart_at + j;
            double r = 0, g = 0, b = 0;
            for (uint32_t q = 0; q < a.n_ranges; ++q) {
                const double* f = fv + ((size_t)q * 3) * Pb;
                r += f[0]; g += f[(size_t)Pb]; b += f[(size_t)Pb * 2];
            }
            drt_f3 px;
            px.x = (float)(r * inv); px.y = (float)(g * inv); px.z = (float)(b * inv);
            *reinterpret_cast<drt_f3_u*>(out + (size_t)e * 3) = px;
        }
        return;
    }
    if (blockIdx.x < film_blocks + grad_words) {
        const int p = (int)(blockIdx.x - film_blocks);
        const int slot = slot_map[p / 3];
        const int src = slot == (int)DRT_SLOT_NONE ? n_rows : (general ? slot * 3 + p % 3 : p);
        double sum = 0;
        for (uint32_t v = 0; v < n_views; ++v) {
            const uint32_t first = views[v].first_block;
            const int view_blocks = (int)views[v].n_blocks;
            double x = 0;
            if (src < n_rows)
                for (int b = threadIdx.x; b < view_blocks; b += DRT_BLOCK)
                    x += gpart[((size_t)first + b) * row_stride + src];
            red[threadIdx.x] = x;
            __syncthreads();
            for (int off = DRT_BLOCK / 2; off > 0; off >>= 1) {
                if ((int)threadIdx.x < off)
                    red[threadIdx.x] += red[threadIdx.x + off];
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                if (view_grads)
                    view_grads[(size_t)v * grad_words + p] = red[0];
                sum = v == 0 ? red[0] : sum + red[0];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0 && grad_sum)
            grad_sum[p] = sum;
        return;
    }
    {
        const uint32_t first = film_blocks + grad_words, nb = gridDim.x - first, me = blockIdx.x - first;
        unsigned long long seg = 0, cap = 0;
        for (uint32_t v = 0; v < n_views; ++v) {
            const uint64_t view_waves = (uint64_t)views[v].n_groups * a.n_ranges;
            const uint32_t* cv = counts + views[v].counts_at;
            for (uint64_t w = (uint64_t)me * DRT_BLOCK + threadIdx.x; w < view_waves; w += (uint64_t)nb * DRT_BLOCK) {
                seg += cv[w];
                cap += cv[view_waves + w];
            }
        }
        for (int off = DRT_WAVE / 2; off > 0; off >>= 1) {
            seg += __shfl_down(seg, off);
            cap += __shfl_down(cap, off);
        }
        if ((threadIdx.x & (DRT_WAVE - 1)) == 0) {
            if (seg) atomicAdd(total, seg);
            if (cap) atomicAdd(total + 3, cap);
        }
    }
}

// ---- the cross-sample normal equations of a frame in the span of K directions (drt_hip_render_normal_equations_cross) -------------
// Behind a launch of k_path's cross-moment form: jpart[range][row][pixel] holds, per pixel of the shard and sample range, 3 nd derivative
// sums (row 3 k + ch), 3 nd moment sums Q_k = sum_s t_{k,s} L_s (row 3 nd + 3 k + ch) and 3 of S2 = sum_s L_s^2 (row 6 nd + ch); fpart the
// radiance sums.  Per channel (blockIdx.y) and pixel, in fp64, every sum over the ranges in range order, n = spp:
//     m = sum L / n      T_k = sum t_k / n      r = m - target
//     bias_k = (Q_k - (sum t_k) m) / ((n - 1) n)        the sample covariance of (t_k, L) over n: what T_k r carries beyond its expectation
//     noise  = (S2 - (sum L) m) / ((n - 1) n)           the sample variance of L over n: the variance of the pixel's mean
//     A[k][l] += T_k T_l (l >= k)     b[k] += T_k r - bias_k     bias[k] += bias_k     loss += r r - noise     bias[K] += noise
// DRT_CROSS_VALUES(NP) running sums per thread, then block_sums; k_cross_eq_finish adds the blocks in a fixed order and mirrors A.  No
// atomics: the same call gives the same bits.  k_normal_eq's grid rule, a pixel per thread.  The derivative images (float, the layout of
// drt_hip_render_tangents: T_k formed as k_normal_eq forms it) and the variance image (noise, H x W x 3) leave in the same pass.
#define DRT_CROSS_VALUES(np) ((np) * ((np) + 1) / 2 + 2 * (np) + 2)
template <int NP>
__global__ void __launch_bounds__(DRT_BLOCK)
k_cross_eq(PathArgs a, const double* __restrict__ jpart, const double* __restrict__ fpart, int n_dirs, const float* __restrict__ target,
           float* __restrict__ out_tan, float* __restrict__ out_var, double* __restrict__ part)
{
    constexpr int NV = DRT_CROSS_VALUES(NP), NT = NP * (NP + 1) / 2;
    const int ch = (int)blockIdx.y;
    const size_t Pb = a.Pb, rows = (size_t)n_dirs * 6 + 3, npix = (size_t)a.W * (size_t)a.H;
    const double n = (double)a.spp, inv = 1.0 / n, inv_pairs = 1.0 / ((n - 1.0) * n);
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k)
        acc[k] = 0.0;
    for (uint32_t j = blockIdx.x * DRT_BLOCK + threadIdx.x; j < a.Pb; j += gridDim.x * DRT_BLOCK) {
        double Ts[NP], Qs[NP], S2 = 0.0, Ls = 0.0;
#pragma unroll
        for (int p = 0; p < NP; ++p)
            Ts[p] = Qs[p] = 0.0;
        for (uint32_t q = 0; q < a.n_ranges; ++q) {
            const double* fj = jpart + ((size_t)q * rows + (size_t)ch) * Pb + j;
#pragma unroll
            for (int p = 0; p < NP; ++p)
                if (p < n_dirs) {
                    Ts[p] += fj[(size_t)(p * 3) * Pb];
                    Qs[p] += fj[((size_t)n_dirs * 3 + (size_t)(p * 3)) * Pb];
                }
            S2 += fj[((size_t)n_dirs * 6) * Pb];
            Ls += fpart[((size_t)q * 3 + (size_t)ch) * Pb + j];
        }
        const size_t gp = path_global_pixel(a, a.p0 + j);
        const double m = Ls * inv, r = m - (double)target[gp * 3 + (size_t)ch];
        const double noise = (S2 - Ls * m) * inv_pairs;
        double T[NP], bias[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            T[p] = Ts[p] * inv;
            bias[p] = (Qs[p] - Ts[p] * m) * inv_pairs;
        }
        if (out_tan) {
#pragma unroll
            for (int p = 0; p < NP; ++p)
                if (p < n_dirs)
                    out_tan[((size_t)p * npix + gp) * 3 + (size_t)ch] = (float)T[p];
        }
        if (out_var)
            out_var[gp * 3 + (size_t)ch] = (float)noise;
        int k = 0;
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int q2 = p; q2 < NP; ++q2)
                acc[k++] += T[p] * T[q2];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            acc[NT + p] += T[p] * r - bias[p];
            acc[NT + NP + p] += bias[p];
        }
        acc[NT + 2 * NP] += r * r - noise;
        acc[NT + 2 * NP + 1] += noise;
    }
    block_sums(acc, part, ((size_t)ch * gridDim.x + blockIdx.x) * NV);
}

// ... its second stage: block (channel, value) adds that value's partials over k_cross_eq's blocks (add_blocks) and writes it where it belongs:
// A[ch][k][l] and its mirror, b[ch][k], bias[ch][k], loss[ch], bias[ch][K], for the n_out directions of the caller (np_w: k_cross_eq's width)
__global__ void __launch_bounds__(DRT_BLOCK)
k_cross_eq_finish(const double* __restrict__ part, int n_blocks, int np_w, int n_out, double* __restrict__ out_A, double* __restrict__ out_b,
                  double* __restrict__ out_loss, double* __restrict__ out_bias)
{
    __shared__ double red[DRT_BLOCK];
    const int nv = DRT_CROSS_VALUES(np_w);
    const int ch = (int)blockIdx.x / nv, k = (int)blockIdx.x - ch * nv;
    add_blocks(red, n_blocks, [&](int b) { return part[((size_t)ch * n_blocks + b) * nv + k]; });
    if (threadIdx.x != 0)
        return;
    const int n_tri = np_w * (np_w + 1) / 2;
    if (k < n_tri) {
        int p = 0, first = 0;                                // row p of the upper triangle starts at `first` and holds np_w - p values
        while (k >= first + (np_w - p)) {
            first += np_w - p;
            ++p;
        }
        const int q = p + (k - first);
        if (p < n_out && q < n_out) {
            out_A[((size_t)ch * n_out + p) * n_out + q] = red[0];
            out_A[((size_t)ch * n_out + q) * n_out + p] = red[0];
        }
    } else if (k < n_tri + np_w) {
        if (k - n_tri < n_out)
            out_b[(size_t)ch * n_out + (k - n_tri)] = red[0];
    } else if (k < n_tri + 2 * np_w) {
        if (out_bias && k - n_tri - np_w < n_out)
            out_bias[(size_t)ch * (n_out + 1) + (k - n_tri - np_w)] = red[0];
    } else if (k == n_tri + 2 * np_w) {
        if (out_loss)
            out_loss[ch] = red[0];
    } else if (out_bias)
        out_bias[(size_t)ch * (n_out + 1) + n_out] = red[0];
}
