// drt_hip.hip -- libdrt_hip.so: the entry points of the C ABI (include/drt_hip.h).  The one translation unit of the library;
// the host runtime behind the entry points is in headers by topic:
//   drt_ctx.h          the context (device, streams, buffers), the state of a render call, helpers
//   drt_tuning.h       every DRT_HIP_* environment variable, read once (listed in INTEGRATION.md section 2)
//   drt_scene.h        upload_scene / update_params: POD scene -> device records, BVH
//   drt_jit.h          k_path compiled for a scene's shape kinds at run time (hiprtc)
//   drt_render_impl.h  one shard's render enqueued: the k_path route and the queue wavefront
//   drt_render.h       a render call in phases; group contexts; asynchronous frames; the all-reduce
// and the kernels in headers by topic too:
//   drt_kernels.h      K1-K5 of the queue wavefront + what all kernels share (RNG, camera, analytic closest hit, BxDF sampler)
//   drt_walk.h         K2 on triangles: the BVH walk
//   drt_backward.h     K6 / K7: the tape's reverse sweep, gradient accumulators, the fixed-order reduction
//   drt_loss.h         the caller's per-sample loss on the tape route: seeds in place, the loss's value
//   drt_chain.h        the unbiased operator's adjoint rounds on the queue wavefront
//   drt_path.h         k_path / k_path_unbiased: the whole path in one launch (analytic scenes)
//   drt_path_mesh.h    k_path_mesh: the same with the BVH walk inside (small frames of mesh scenes)
#include "drt_kernels.h"
#include "drt_walk.h"
#include "drt_backward.h"
#include "drt_loss.h"
#include "drt_chain.h"
#include "drt_path.h"
#include "drt_path_mesh.h"
#include "drt_bvh.h"
#include "drt_jit.h"

#include <rccl/rccl.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>


#include "drt_tuning.h"
#include "drt_pixels.h"
#include "drt_ctx.h"
#include "drt_scene.h"
#include "drt_render_impl.h"
#include "drt_render.h"

extern "C" {

int drt_hip_abi_version(void) { return DRT_HIP_ABI_VERSION; }

int drt_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int drt_hip_create(int device_id, drt_hip_ctx** out)
{
    if (!out)
        return DRT_ERR_INVALID;
    *out = nullptr;
    int n = drt_hip_device_count();
    if (n <= 0 || device_id < 0 || device_id >= n)
        return DRT_ERR_NO_DEVICE;
    if (hipSetDevice(device_id) != hipSuccess)
        return DRT_ERR_NO_DEVICE;
    drt_hip_ctx* ctx = new drt_hip_ctx();
    ctx->device = device_id;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) {
        ctx->n_cu = prop.multiProcessorCount;
        ctx->device_mem = (uint64_t)prop.totalGlobalMem;
        if (prop.gcnArchName[0])
            ctx->arch = prop.gcnArchName;
    }
    ctx->jit_mode = tuning().jit;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return DRT_ERR_HIP;
    }
    {   // Every stream of the context is made HERE, in this order, before the process makes any other: which of them run
        // side by side depends on the order HIP has seen them in (measured: the two k_path streams made later, next to the
        // copy stream, never overlapped their grids; made here they do -- and the copy stream made later, after them, no
        // longer overlapped its launch with the next frame: 0.81 -> 0.90 ms through host buffers).
        for (int i = 0; i < 2 && tuning().overlap_frames; ++i)
            if (hipStreamCreateWithFlags(&ctx->path_stream[i], hipStreamNonBlocking) != hipSuccess)
                ctx->path_stream[i] = nullptr;
        if (!ctx->path_stream[1]) ctx->path_stream[0] = nullptr;
        // (highest priority: the copies and the all-reduce of frame i must not queue behind the kernels of frame i + 1)
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (hipStreamCreateWithPriority(&ctx->copy_stream, hipStreamNonBlocking, greatest) != hipSuccess)
            ctx->copy_stream = nullptr;
        for (int i = 0; i < 2; ++i)
            if (hipEventCreateWithFlags(&ctx->ev_lane_free[i], hipEventDisableTiming) != hipSuccess)
                ctx->ev_lane_free[i] = nullptr;
        if (hipEventCreateWithFlags(&ctx->ev_params, hipEventDisableTiming) != hipSuccess)
            ctx->ev_params = nullptr;
    }
    {   // the BVH walk is a persistent kernel whose waves own strided streams of rays: its grid must be exactly what
        // is resident at once (more blocks would run as a second round behind the first, at half the occupancy)
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_intersect_mesh<float>, DRT_BLOCK, 0) == hipSuccess && nb > 0)
            ctx->mesh_blocks_per_cu = nb;
        (void)hipGetLastError();
        if (tuning().mesh_blocks_per_cu > 0)
            ctx->mesh_blocks_per_cu = tuning().mesh_blocks_per_cu;
    }
    *out = ctx;
    return DRT_OK;
}

void drt_hip_destroy(drt_hip_ctx* ctx)
{
    if (!ctx)
        return;
    if (!ctx->members.empty() || !ctx->stream) {          // a group context owns members, nothing else
        for (drt_hip_ctx* m : ctx->members)
            drt_hip_destroy(m);
        delete ctx;
        return;
    }
    (void)hipSetDevice(ctx->device);
    if (ctx->stream)
        (void)hipStreamSynchronize(ctx->stream);
    if (ctx->copy_stream)
        (void)hipStreamSynchronize(ctx->copy_stream);
    if (ctx->comm)
        (void)ncclCommDestroy(ctx->comm);
    if (ctx->ev_done)
        (void)hipEventDestroy(ctx->ev_done);
    DevBuf* bufs[] = {&ctx->hist_ovf[0], &ctx->hist_ovf[1], &ctx->mesh_ovf[0], &ctx->mesh_ovf[1], &ctx->fpart2, &ctx->gpart2, &ctx->counts2, &ctx->fpart, &ctx->gpix, &ctx->cand[0], &ctx->cand[1], &ctx->cand_a[0], &ctx->cand_a[1], &ctx->cand_b[0], &ctx->cand_b[1], &ctx->cand_count[0], &ctx->cand_count[1], &ctx->ray_a[0], &ctx->ray_a[1], &ctx->ray_a[2], &ctx->ray_b[0], &ctx->ray_b[1], &ctx->ray_b[2], &ctx->ray_id[0], &ctx->ray_id[1], &ctx->ray_id[2], &ctx->hit, &ctx->hit2, &ctx->hit3, &ctx->lacc, &ctx->gpath, &ctx->gfilm, &ctx->gimg_out, &ctx->tape, &ctx->nv,
                      &ctx->ch_cva, &ctx->ch_cvb, &ctx->ch_cvh, &ctx->ch_nxa, &ctx->ch_nxb, &ctx->ch_nxh, &ctx->ch_g,
                      &ctx->ch_w, &ctx->ch_ids, &ctx->ch_ndraw, &ctx->ch_dbase, &ctx->counts, &ctx->film, &ctx->gpart, &ctx->adjoint, &ctx->tangent,
                      &ctx->neq_part, &ctx->neq_out, &ctx->neq_in, &ctx->neq_jac, &ctx->neq_rgb, &ctx->loss_part, &ctx->loss_out};
    for (DevBuf* b : bufs)
        release(*b);
    for (int i = 0; i < DRT_HIP_FRAMES_IN_FLIGHT; ++i) {
        release(ctx->segtotal[i]);
        release(ctx->grad[i]);
        release(ctx->out[i]);
    }
    release_mesh(ctx);
    for (hipModule_t m : ctx->jit_modules)
        (void)hipModuleUnload(m);
    drt_jit::wait_idle();                   // (a compile this context started in the background is allowed to finish)
    if (ctx->d_scene_f) (void)hipFree(ctx->d_scene_f);
    if (ctx->d_scene_d) (void)hipFree(ctx->d_scene_d);
    if (ctx->d_params_f) (void)hipFree(ctx->d_params_f);
    if (ctx->d_params_d) (void)hipFree(ctx->d_params_d);
    if (ctx->h_probe)
        (void)hipHostFree(ctx->h_probe);
    if (ctx->h_params)
        (void)hipHostFree(ctx->h_params);
    for (int i = 0; i < 2; ++i) {
        if (ctx->h_tangent[i]) (void)hipHostFree(ctx->h_tangent[i]);
        if (ctx->ev_tangent[i]) (void)hipEventDestroy(ctx->ev_tangent[i]);
    }
    for (const drt_hip_ctx::PinnedRange& r : ctx->pinned)
        (void)hipHostUnregister(r.host);
    for (int i = 0; i < DRT_HIP_FRAMES_IN_FLIGHT; ++i) {
        if (ctx->h_stage[i])
            (void)hipHostFree(ctx->h_stage[i]);
        if (ctx->ev_rendered[i]) (void)hipEventDestroy(ctx->ev_rendered[i]);
        if (ctx->ev_copied[i]) (void)hipEventDestroy(ctx->ev_copied[i]);
    }
    if (ctx->copy_stream)
        (void)hipStreamDestroy(ctx->copy_stream);
    for (int i = 0; i < 2; ++i) {
        if (ctx->path_stream[i]) { (void)hipStreamSynchronize(ctx->path_stream[i]); (void)hipStreamDestroy(ctx->path_stream[i]); }
        if (ctx->ev_begin[i]) (void)hipEventDestroy(ctx->ev_begin[i]);
        if (ctx->ev_path[i]) (void)hipEventDestroy(ctx->ev_path[i]);
        if (ctx->ev_lane_free[i]) (void)hipEventDestroy(ctx->ev_lane_free[i]);
    }
    if (ctx->ev_params) (void)hipEventDestroy(ctx->ev_params);
    release(ctx->probe);
    for (hipEvent_t e : ctx->event_pool)
        (void)hipEventDestroy(e);
    if (ctx->stream)
        (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

} // extern "C"

extern "C" {

// ---- caller buffers the finishing kernels write directly (ABI v7) -----------------------------------------------------
int drt_hip_pin_host(drt_hip_ctx* ctx, void* ptr, size_t bytes)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    if (!ctx->members.empty())
        return fail(ctx, DRT_ERR_UNSUPPORTED, "pin_host: not on a group context");
    if (!ptr || bytes == 0)
        return fail(ctx, DRT_ERR_INVALID, "pin_host: NULL or empty range");
    for (const drt_hip_ctx::PinnedRange& r : ctx->pinned)
        if ((uint8_t*)ptr < r.host + r.bytes && r.host < (uint8_t*)ptr + bytes)
            return fail(ctx, DRT_ERR_INVALID, "pin_host: the range overlaps one that is pinned already");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipHostRegister(ptr, bytes, hipHostRegisterMapped | hipHostRegisterPortable));
    void* dev = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&dev, ptr, 0);
    if (e != hipSuccess || !dev) {
        (void)hipHostUnregister(ptr);
        (void)hipGetLastError();
        return fail(ctx, DRT_ERR_HIP, "pin_host: the range cannot be mapped into the device's address space");
    }
    ctx->pinned.push_back({(uint8_t*)ptr, bytes, (uint8_t*)dev});
    return DRT_OK;
}

int drt_hip_unpin_host(drt_hip_ctx* ctx, void* ptr)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    for (size_t i = 0; i < ctx->pinned.size(); ++i)
        if (ctx->pinned[i].host == (uint8_t*)ptr) {
            for (int f = 0; f < DRT_HIP_FRAMES_IN_FLIGHT; ++f)
                if (ctx->in_flight[f])
                    return fail(ctx, DRT_ERR_INVALID, "unpin_host: asynchronous frames are in flight -- drt_hip_wait for them first");
            HIPCHK(ctx, hipSetDevice(ctx->device));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            HIPCHK(ctx, hipHostUnregister(ptr));
            ctx->pinned.erase(ctx->pinned.begin() + (long)i);
            return DRT_OK;
        }
    return fail(ctx, DRT_ERR_INVALID, "unpin_host: not the start of a pinned range");
}

int drt_hip_render(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp,
                   const float* adjoint_rgb, float* out_rgb, double* out_param_grad, drt_hip_stats* stats)
{
    return render_common(ctx, cam, rp, adjoint_rgb, out_rgb, out_param_grad, stats, -1, nullptr);
}

int drt_hip_render_gradient_image(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp,
                                  int32_t param, const float* adjoint_rgb, float* out_rgb, float* out_grad_rgb,
                                  drt_hip_stats* stats)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    drt_hip_ctx* first = ctx->members.empty() ? ctx : ctx->members[0];
    if (!first->has_scene)
        return fail(ctx, DRT_ERR_NO_SCENE, "render before upload_scene");
    if (!rp || !out_grad_rgb || param < 0 || param >= first->n_user_params)
        return fail(ctx, DRT_ERR_INVALID, "gradient image: bad parameter index or NULL output");
    drt_render_params r = *rp;
    r.flags |= DRT_RENDER_BACKWARD;
    return render_common(ctx, cam, &r, adjoint_rgb, out_rgb, nullptr, stats, param, out_grad_rgb);
}

} // extern "C"

// ---- the renders that exist on the one-launch path kernel's special forms only: forward mode along one direction, the Jacobian form,
// K directions, K parameter sets.  What they share: the rows behind the kernel's `params`, the refusals, the K images' way back ----
// dst = [the scene's parameters | row_1 | ... | row_K] in compute type R.  Rows at and above n_rows (padding up to the kernel's width) and the
// internal constants (a mirror's colour) of every row are padded by one of three rules
enum class RowPad : int {
    zero,                       // directions
    own,                        // sets: the context's own parameters
    own_even,                   // rows in PAIRS (a set, then its direction: drt_hip_render_param_sets_along): even rows like sets, odd rows like directions
};
template <typename R>
__global__ void __launch_bounds__(DRT_BLOCK) k_stage_rows(const R* __restrict__ params, int n_all, const double* __restrict__ h_rows, int n_user,
                                                          int n_rows, int K, RowPad pad, R* __restrict__ dst)
{
    for (int i = blockIdx.x * DRT_BLOCK + threadIdx.x; i < n_all; i += gridDim.x * DRT_BLOCK) {
        const R own = params[i];
        dst[i] = own;
        for (int k = 0; k < K; ++k)
            dst[(size_t)(1 + k) * n_all + i] = (k < n_rows && i < n_user) ? (R)h_rows[(size_t)k * n_user + i]
                                               : ((pad == RowPad::own || (pad == RowPad::own_even && !(k & 1))) ? own : R(0));
    }
}

// the caller's n_rows x n_user rows -> pinned memory -> ctx->tangent.p = [parameters | row_1 | ... | row_K], in stream order.  Two pinned
// copies used in turn: the one this call rewrites was read by the launch of the call before the previous one, and its event says so
// (rows2: the rows come in pairs -- row 2 k from `rows`, row 2 k + 1 from `rows2`, n_rows and K counting both)
static int stage_rows(drt_hip_ctx* ctx, const drt_render_params* rp, const double* rows, int n_rows, int K, RowPad pad, const double* rows2 = nullptr)
{
    const int n_user = ctx->n_user_params * 3, n_all = ctx->n_params * 3;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int hb = (int)(ctx->tangent_calls++ & 1);
    const size_t need = (size_t)n_rows * (size_t)(n_user ? n_user : 1);
    if (!ctx->ev_tangent[hb])
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_tangent[hb], hipEventDisableTiming));
    else
        HIPCHK(ctx, hipEventSynchronize(ctx->ev_tangent[hb]));
    if (ctx->h_tangent_cap[hb] < need) {
        if (ctx->h_tangent[hb])
            (void)hipHostFree(ctx->h_tangent[hb]);
        ctx->h_tangent[hb] = nullptr;
        ctx->h_tangent_cap[hb] = 0;
        HIPCHK(ctx, hipHostMalloc((void**)&ctx->h_tangent[hb], need * sizeof(double)));
        ctx->h_tangent_cap[hb] = need;
    }
    if (rows2)
        for (int k = 0; k < n_rows; ++k)
            memcpy(ctx->h_tangent[hb] + (size_t)k * (size_t)n_user, ((k & 1) ? rows2 : rows) + (size_t)(k >> 1) * (size_t)n_user, (size_t)n_user * sizeof(double));
    else
        memcpy(ctx->h_tangent[hb], rows, (size_t)n_rows * (size_t)n_user * sizeof(double));
    int rc;
    if ((rc = ensure(ctx, ctx->tangent, (size_t)(n_all ? n_all : 1) * (size_t)(1 + K) * sizeof(double))) != DRT_OK) return rc;
    if (n_all > 0) {
        const unsigned blocks = (unsigned)((n_all + DRT_BLOCK - 1) / DRT_BLOCK);
        if (rp->flags & DRT_RENDER_F64)
            hipLaunchKernelGGL(k_stage_rows<double>, dim3(blocks), dim3(DRT_BLOCK), 0, ctx->stream, (const double*)ctx->d_params_d, n_all,
                               (const double*)ctx->h_tangent[hb], n_user, n_rows, K, pad, (double*)ctx->tangent.p);
        else
            hipLaunchKernelGGL(k_stage_rows<float>, dim3(blocks), dim3(DRT_BLOCK), 0, ctx->stream, (const float*)ctx->d_params_f, n_all,
                               (const double*)ctx->h_tangent[hb], n_user, n_rows, K, pad, (float*)ctx->tangent.p);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev_tangent[hb], ctx->stream));
    return DRT_OK;
}

// who is asking, and the few words of the shared refusals that are its own
struct PathFormCaller {
    const char* who;            // every message's first words
    const char* group_hint;     // what to do on a group context instead
    const char* what;           // "... -- `what` on the one-launch path kernel, one context"
    int cap;                    // the most parameters (internal constants included) its form of the kernel takes ...
    const char* above_cap;      // ... and what it says above that
};

// a refusal in the caller's name
static int refuse(drt_hip_ctx* ctx, const PathFormCaller& c, int code, const std::string& what)
{
    return fail(ctx, code, (std::string(c.who) + ": " + what).c_str());
}

// The refusals the Jacobian, K-direction and parameter-set forms share, in the order they have always come in: the context, the scene and the
// camera (refuse_before); the entry point's own checks; then what the one-launch path kernel over the whole shard in one batch cannot do
// (refuse_after).  (drt_hip_render_tangent is older, renders in batches and speaks its own words: it keeps its own ladder.)
static int refuse_before(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, const PathFormCaller& c)
{
    if (!ctx->members.empty())
        return refuse(ctx, c, DRT_ERR_UNSUPPORTED, std::string("not on a group context (") + c.group_hint + ")");
    if (!ctx->has_scene)
        return fail(ctx, DRT_ERR_NO_SCENE, "render before upload_scene");
    if (!cam || !rp || cam->width <= 0 || cam->height <= 0)
        return refuse(ctx, c, DRT_ERR_INVALID, "bad camera or render parameters");
    return DRT_OK;
}

static int refuse_after(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, const PathFormCaller& c)
{
    for (int i = 0; i < DRT_HIP_FRAMES_IN_FLIGHT; ++i)
        if (ctx->in_flight[i])
            return refuse(ctx, c, DRT_ERR_INVALID, "asynchronous frames are in flight -- drt_hip_wait for them first");
    if (rp->flags & (DRT_RENDER_UNFUSED | DRT_RENDER_UNBIASED | DRT_RENDER_LOSS_L2 | DRT_RENDER_ALLREDUCE | DRT_RENDER_ALLREDUCE_ASYNC))
        return refuse(ctx, c, DRT_ERR_UNSUPPORTED, std::string("not with DRT_RENDER_UNFUSED, _UNBIASED, _LOSS_L2 or _ALLREDUCE* -- ") + c.what +
                                                   " on the one-launch path kernel, one context");
    if (ctx->has_mesh)
        return refuse(ctx, c, DRT_ERR_UNSUPPORTED, "not of a scene that holds a triangle mesh");
    if (rp->bounces_per_launch >= 1)
        return refuse(ctx, c, DRT_ERR_UNSUPPORTED, "they come from the one-launch path kernel -- not with bounces_per_launch >= 1");
    if (ctx->n_params > c.cap)
        return refuse(ctx, c, DRT_ERR_UNSUPPORTED, c.above_cap);
    if ((uint64_t)cam->width * (uint64_t)cam->height * (uint64_t)(rp->spp > 0 ? rp->spp : 1) > 0x7FFFFFFFull)
        return refuse(ctx, c, DRT_ERR_UNSUPPORTED, "more than 2^31 camera samples in one frame (the shard renders in one batch)");
    return DRT_OK;
}

static int render_tangent_common(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, const double* param_tangent,
                                 float* out_rgb, float* out_tangent_rgb, drt_hip_stats* stats, bool keep_sums)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    if (!ctx->members.empty())
        return fail(ctx, DRT_ERR_UNSUPPORTED, "render_tangent: not on a group context");
    if (!ctx->has_scene)
        return fail(ctx, DRT_ERR_NO_SCENE, "render before upload_scene");
    if (!rp || !param_tangent)
        return fail(ctx, DRT_ERR_INVALID, "render_tangent: NULL render parameters, tangent or output");
    if (rp->flags & (DRT_RENDER_BACKWARD | DRT_RENDER_UNBIASED | DRT_RENDER_LOSS_L2 | DRT_RENDER_ALLREDUCE | DRT_RENDER_ALLREDUCE_ASYNC))
        return fail(ctx, DRT_ERR_INVALID, "render_tangent: forward mode takes no reverse-mode flag (DRT_RENDER_BACKWARD, _UNBIASED, _LOSS_L2, _ALLREDUCE*)");
    for (int i = 0; i < ctx->n_user_params * 3; ++i)
        if (!std::isfinite(param_tangent[i]))
            return fail(ctx, DRT_ERR_INVALID, "render_tangent: the tangent holds a value that is not finite");
    for (int i = 0; i < DRT_HIP_FRAMES_IN_FLIGHT; ++i)
        if (ctx->in_flight[i])
            return fail(ctx, DRT_ERR_INVALID, "render: asynchronous frames are in flight -- drt_hip_wait for them first");
    if (ctx->has_mesh)
        return fail(ctx, DRT_ERR_UNSUPPORTED, "render_tangent: no tangent image of a scene that holds a triangle mesh");
    if (rp->bounces_per_launch >= 1 || (rp->flags & DRT_RENDER_UNFUSED))
        return fail(ctx, DRT_ERR_UNSUPPORTED, "render_tangent: the tangent image comes from the one-launch path kernel -- not with bounces_per_launch >= 1 "
                                              "or DRT_RENDER_UNFUSED");
    if (ctx->n_params > DRT_PATH_LDS_PARAMS)
        return fail(ctx, DRT_ERR_UNSUPPORTED, "render_tangent: a tangent of more parameters than the path kernels stage (136)");
    int rc;
    if ((rc = stage_rows(ctx, rp, param_tangent, 1, 1, RowPad::zero)) != DRT_OK) return rc;
    TangentRequest req;
    req.kind = TangentRequest::Kind::forward;
    req.d_params = ctx->tangent.p;
    req.keep_sums = keep_sums;
    return render_common(ctx, cam, rp, nullptr, out_rgb, nullptr, stats, -1, out_tangent_rgb, &req);
}

// the call behind its refusals, for P rows -- the scene's parameters (the Jacobian form) or the directions of req (the K-direction forward
// form): the caller's images to the device, the render, the sums and the P images back.  Without a target and a residual (the tangent
// images alone) the reduction runs on a zero residual; without out_A its sums stay in the context.
// (cross: drt_hip_render_normal_equations_cross -- the sums gain out_bias, 3 x (P + 1), behind the loss, the images out_variance behind the P)
static int normal_equations_run(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, const float* target_rgb,
                                const float* residual_rgb, float* out_rgb, double* out_A, double* out_b, double* out_loss,
                                float* out_jacobian, drt_hip_stats* stats, size_t P, TangentRequest& req, const char* who,
                                bool cross = false, double* out_bias = nullptr, float* out_variance = nullptr)
{
    const bool dev = (rp->flags & DRT_RENDER_DEVICE_OUT) != 0;
    const size_t npix = (size_t)cam->width * (size_t)cam->height;
    const size_t nA = 3 * P * P, nb = 3 * P, nbias = cross ? 3 * (P + 1) : 0;
    const float* src = target_rgb ? target_rgb : residual_rgb;
    if (!dev && src)
        for (size_t i = 0; i < npix * 3; ++i)
            if (!std::isfinite(src[i]))
                return fail(ctx, DRT_ERR_INVALID, (std::string(who) + ": the target / residual image holds a value that is not finite").c_str());
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    NormalEqRequest q;
    float* rgb = out_rgb;
    if (!src || !dev) {
        if ((rc = ensure(ctx, ctx->neq_in, npix * 3 * sizeof(float))) != DRT_OK) return rc;
        if (!src)
            HIPCHK(ctx, hipMemsetAsync(ctx->neq_in.p, 0, npix * 3 * sizeof(float), ctx->stream));
    }
    if (!dev || !out_A) {
        if ((rc = ensure(ctx, ctx->neq_out, (nA + nb + 3 + nbias) * sizeof(double))) != DRT_OK) return rc;
        q.d_A = (double*)ctx->neq_out.p; q.d_b = q.d_A + nA; q.d_loss = q.d_b + nb;
        if (cross) q.d_bias = q.d_loss + 3;
    }
    q.cross = cross;
    if (dev) {
        if (out_A) {
            q.d_A = out_A; q.d_b = out_b; q.d_loss = out_loss;
            if (cross) q.d_bias = out_bias;
        }
        q.d_jacobian = out_jacobian;
        q.d_variance = out_variance;
        if (!rgb) {       // (the radiance sums are part of the pipeline: an image of the context's own)
            if ((rc = ensure(ctx, ctx->neq_rgb, npix * 3 * sizeof(float))) != DRT_OK) return rc;
            rgb = (float*)ctx->neq_rgb.p;
        }
        if (!src)
            src = (const float*)ctx->neq_in.p;
    } else {
        if (src)
            HIPCHK(ctx, hipMemcpyAsync(ctx->neq_in.p, src, npix * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        src = (const float*)ctx->neq_in.p;
        if (out_jacobian || out_variance) {
            if ((rc = ensure(ctx, ctx->neq_jac, ((P ? P : 1) + (out_variance ? 1 : 0)) * npix * 3 * sizeof(float))) != DRT_OK) return rc;
            if (out_jacobian) q.d_jacobian = (float*)ctx->neq_jac.p;
            if (out_variance) q.d_variance = (float*)ctx->neq_jac.p + (P ? P : 1) * npix * 3;
        }
        if (!rgb) {
            ctx->tangent_rgb32.resize(npix * 3);
            rgb = ctx->tangent_rgb32.data();
        }
    }
    (target_rgb ? q.d_target : q.d_residual) = src;
    // (a shard without rows launches nothing: its sums are zero)
    if (nA) HIPCHK(ctx, hipMemsetAsync(q.d_A, 0, nA * sizeof(double), ctx->stream));
    if (nb) HIPCHK(ctx, hipMemsetAsync(q.d_b, 0, nb * sizeof(double), ctx->stream));
    if (q.d_loss) HIPCHK(ctx, hipMemsetAsync(q.d_loss, 0, 3 * sizeof(double), ctx->stream));
    if (q.d_bias) HIPCHK(ctx, hipMemsetAsync(q.d_bias, 0, nbias * sizeof(double), ctx->stream));
    drt_render_params r = *rp;
    r.flags &= ~(uint32_t)DRT_RENDER_BACKWARD;       // (the Jacobian needs no seed and no summed gradient)
    req.neq = &q;
    if ((rc = render_common(ctx, cam, &r, nullptr, rgb, nullptr, stats, -1, nullptr, &req)) != DRT_OK)
        return rc;
    if (dev)
        return DRT_OK;
    // host buffers: the render has waited for its stream; a few hundred bytes of sums, and the Jacobian's rows of this shard where asked for
    std::vector<double> sums(nA + nb + 3 + nbias);
    HIPCHK(ctx, hipMemcpy(sums.data(), ctx->neq_out.p, sums.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (nA && out_A) memcpy(out_A, sums.data(), nA * sizeof(double));
    if (nb && out_b) memcpy(out_b, sums.data() + nA, nb * sizeof(double));
    if (out_loss) memcpy(out_loss, sums.data() + nA + nb, 3 * sizeof(double));
    if (out_bias && nbias) memcpy(out_bias, sums.data() + nA + nb + 3, nbias * sizeof(double));
    if ((out_jacobian || out_variance) && P) {
        const RenderJob& j = ctx->job;
        ctx->neq_host.resize((P + (out_variance ? 1 : 0)) * npix * 3);
        HIPCHK(ctx, hipMemcpy(ctx->neq_host.data(), ctx->neq_jac.p, ctx->neq_host.size() * sizeof(float), hipMemcpyDeviceToHost));
        const size_t row = (size_t)cam->width * 3;
        // (image P: the variance image behind the P rows' images)
        for (size_t p = out_jacobian ? 0 : P; p < P + (out_variance ? 1 : 0); ++p)
            for_each_band(cam->height, j.band, j.n_shards, j.shard, [&](int y0, int y1) {
                memcpy((p < P ? out_jacobian + p * npix * 3 : out_variance) + (size_t)y0 * row, ctx->neq_host.data() + p * npix * 3 + (size_t)y0 * row,
                       (size_t)(y1 - y0) * row * sizeof(float));
            });
    }
    return DRT_OK;
}

extern "C" {

int drt_hip_render_tangent(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, const double* param_tangent,
                           float* out_rgb, float* out_tangent_rgb, drt_hip_stats* stats)
{
    if (ctx && !out_tangent_rgb)
        return fail(ctx, DRT_ERR_INVALID, "render_tangent: NULL render parameters, tangent or output");
    return render_tangent_common(ctx, cam, rp, param_tangent, out_rgb, out_tangent_rgb, stats, false);
}

int drt_hip_render_tangent_double(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, const double* param_tangent,
                                  double* out_rgb, double* out_tangent_rgb, drt_hip_stats* stats)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    if (!out_tangent_rgb)
        return fail(ctx, DRT_ERR_INVALID, "render_tangent: NULL render parameters, tangent or output");
    if (rp && (rp->flags & DRT_RENDER_DEVICE_OUT))
        return fail(ctx, DRT_ERR_INVALID, "render_tangent_double: host buffers only");
    if (!cam || cam->width <= 0 || cam->height <= 0)
        return fail(ctx, DRT_ERR_INVALID, "render: bad camera or render parameters");
    // The render goes the way of a frame in several batches: both images' sums are gathered in `film` / `gfilm`, in double, and are
    // fetched from there.  The float tangent image is resolved on the device and goes nowhere; the float image is what makes the
    // pipeline keep radiance sums at all: it goes to a frame of the context's own.
    float* rgb32 = nullptr;
    if (out_rgb) {
        ctx->tangent_rgb32.resize((size_t)cam->width * (size_t)cam->height * 3);
        rgb32 = ctx->tangent_rgb32.data();
    }
    int rc = render_tangent_common(ctx, cam, rp, param_tangent, rgb32, nullptr, stats, true);
    if (rc != DRT_OK)
        return rc;
    const RenderJob& j = ctx->job;
    const size_t row = (size_t)cam->width * 3;
    const double inv = 1.0 / (double)rp->spp;
    std::vector<double> sums((size_t)j.n_local_pixels * 3);
    auto fetch = [&](const DevBuf& src, double* dst) -> int {
        if (!sums.empty())
            HIPCHK(ctx, hipMemcpy(sums.data(), src.p, sums.size() * sizeof(double), hipMemcpyDeviceToHost));
        size_t local = 0;                 // (the shard's rows in band order: how the kernels number its pixels)
        for_each_band(cam->height, j.band, j.n_shards, j.shard, [&](int y0, int y1) {
            for (size_t i = (size_t)y0 * row; i < (size_t)y1 * row; ++i)
                dst[i] = sums[local++] * inv;
        });
        return DRT_OK;
    };
    if ((rc = fetch(ctx->gfilm, out_tangent_rgb)) != DRT_OK) return rc;
    if (out_rgb && (rc = fetch(ctx->film, out_rgb)) != DRT_OK) return rc;
    return DRT_OK;
}


// ---- the Gauss-Newton normal equations of a frame: the path kernel's Jacobian form, then k_normal_eq (drt_path.h) ----
int drt_hip_render_normal_equations(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, const float* target_rgb,
                                    const float* residual_rgb, float* out_rgb, double* out_A, double* out_b, double* out_loss,
                                    float* out_jacobian, drt_hip_stats* stats)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    const PathFormCaller me = {"normal equations", "render the shards on plain contexts and add them", "the biased operator", DRT_FAST_PARAMS,
                               ctx->n_user_params > DRT_FAST_PARAMS
        ? "more than DRT_FAST_PARAMS = 8 parameters (the Jacobian is the path kernel's gradient "
          "columns, which stop there; J^T J v by drt_hip_render_tangent + drt_hip_render is the matrix-free route)"
        : "the scene's parameters and the constant a mirror material adds take more than DRT_FAST_PARAMS = 8 "
          "gradient columns of the path kernel (a mirror costs one: at most 7 parameters beside it)"};
    int rc;
    if ((rc = refuse_before(ctx, cam, rp, me)) != DRT_OK) return rc;
    if ((target_rgb != nullptr) == (residual_rgb != nullptr))
        return refuse(ctx, me, DRT_ERR_INVALID, "exactly one of target_rgb and residual_rgb");
    if (!out_A || !out_b)
        return refuse(ctx, me, DRT_ERR_INVALID, "NULL out_A or out_b");
    if ((rc = refuse_after(ctx, cam, rp, me)) != DRT_OK) return rc;
    TangentRequest req;
    req.kind = TangentRequest::Kind::jacobian;
    return normal_equations_run(ctx, cam, rp, target_rgb, residual_rgb, out_rgb, out_A, out_b, out_loss, out_jacobian, stats,
                                (size_t)ctx->n_user_params, req, "normal equations");
}


} // extern "C"

// ---- J V for up to DRT_HIP_MAX_DIRS directions in one render, and the normal equations in their span ----
static int render_tangents_common(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_dirs,
                                  const double* param_tangents, const float* target_rgb, const float* residual_rgb, float* out_rgb,
                                  double* out_A, double* out_b, double* out_loss, float* out_tangents, drt_hip_stats* stats, bool along)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    const PathFormCaller me = {along ? "normal equations along" : "tangents", "render the shards on plain contexts", "forward mode", DRT_PATH_LDS_PARAMS,
                               "more parameters than the path kernels stage (136)"};
    int rc;
    if ((rc = refuse_before(ctx, cam, rp, me)) != DRT_OK) return rc;
    if (n_dirs < 1 || n_dirs > DRT_HIP_MAX_DIRS)
        return refuse(ctx, me, DRT_ERR_INVALID, "n_dirs outside 1 ... DRT_HIP_MAX_DIRS = 8");
    if (!param_tangents || (along ? (!out_A || !out_b) : !out_tangents))
        return refuse(ctx, me, DRT_ERR_INVALID, "NULL directions or output");
    if (along && (target_rgb != nullptr) == (residual_rgb != nullptr))
        return refuse(ctx, me, DRT_ERR_INVALID, "exactly one of target_rgb and residual_rgb");
    for (size_t i = 0; i < (size_t)n_dirs * (size_t)ctx->n_user_params * 3; ++i)
        if (!std::isfinite(param_tangents[i]))
            return refuse(ctx, me, DRT_ERR_INVALID, "a direction holds a value that is not finite");
    if ((rc = refuse_after(ctx, cam, rp, me)) != DRT_OK) return rc;
    // (directions at and above n_dirs, up to the kernel's width, are zero)
    if ((rc = stage_rows(ctx, rp, param_tangents, n_dirs, n_dirs <= 2 ? 2 : (n_dirs <= 4 ? 4 : 8), RowPad::zero)) != DRT_OK) return rc;
    TangentRequest req;
    req.kind = TangentRequest::Kind::directions;
    req.d_params = ctx->tangent.p;
    req.n_dirs = n_dirs;
    return normal_equations_run(ctx, cam, rp, target_rgb, residual_rgb, out_rgb, out_A, out_b, out_loss, out_tangents, stats, (size_t)n_dirs, req,
                                me.who);
}

// ---- ... and the cross-sample normal equations: b and the loss as U-statistics over each pixel's samples, unbiased from ONE render ----
static int render_cross_common(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_dirs,
                               const double* param_tangents, const float* target_rgb, float* out_rgb, double* out_A, double* out_b,
                               double* out_loss, double* out_bias, float* out_tangents, float* out_variance_rgb, drt_hip_stats* stats)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    const PathFormCaller me = {"normal equations cross", "render the shards on plain contexts", "forward mode", DRT_PATH_LDS_PARAMS,
                               "more parameters than the path kernels stage (136)"};
    int rc;
    if ((rc = refuse_before(ctx, cam, rp, me)) != DRT_OK) return rc;
    if (rp->spp < 2)
        return refuse(ctx, me, DRT_ERR_INVALID, "spp < 2 (the estimator needs a pair of samples per pixel)");
    if (n_dirs < 1 || n_dirs > DRT_HIP_MAX_DIRS_CROSS)
        return refuse(ctx, me, DRT_ERR_INVALID, "n_dirs outside 1 ... DRT_HIP_MAX_DIRS_CROSS = 8");
    if (!param_tangents || !target_rgb || !out_A || !out_b || !out_loss)
        return refuse(ctx, me, DRT_ERR_INVALID, "NULL directions, target_rgb, out_A, out_b or out_loss");
    for (size_t i = 0; i < (size_t)n_dirs * (size_t)ctx->n_user_params * 3; ++i)
        if (!std::isfinite(param_tangents[i]))
            return refuse(ctx, me, DRT_ERR_INVALID, "a direction holds a value that is not finite");
    if ((rc = refuse_after(ctx, cam, rp, me)) != DRT_OK) return rc;
    // (directions at and above n_dirs, up to the kernel's width, are zero)
    if ((rc = stage_rows(ctx, rp, param_tangents, n_dirs, n_dirs <= 2 ? 2 : (n_dirs <= 4 ? 4 : 8), RowPad::zero)) != DRT_OK) return rc;
    TangentRequest req;
    req.kind = TangentRequest::Kind::directions;
    req.d_params = ctx->tangent.p;
    req.n_dirs = n_dirs;
    return normal_equations_run(ctx, cam, rp, target_rgb, nullptr, out_rgb, out_A, out_b, out_loss, out_tangents, stats, (size_t)n_dirs, req,
                                me.who, true, out_bias, out_variance_rgb);
}

extern "C" {

int drt_hip_render_normal_equations_cross(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_dirs,
                                          const double* param_tangents, const float* target_rgb, float* out_rgb, double* out_A, double* out_b,
                                          double* out_loss, double* out_bias, float* out_tangents, float* out_variance_rgb, drt_hip_stats* stats)
{
    return render_cross_common(ctx, cam, rp, n_dirs, param_tangents, target_rgb, out_rgb, out_A, out_b, out_loss, out_bias, out_tangents,
                               out_variance_rgb, stats);
}

int drt_hip_render_tangents(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_dirs,
                            const double* param_tangents, float* out_rgb, float* out_tangents, drt_hip_stats* stats)
{
    return render_tangents_common(ctx, cam, rp, n_dirs, param_tangents, nullptr, nullptr, out_rgb, nullptr, nullptr, nullptr, out_tangents, stats, false);
}

int drt_hip_render_normal_equations_along(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_dirs,
                                          const double* param_tangents, const float* target_rgb, const float* residual_rgb, float* out_rgb,
                                          double* out_A, double* out_b, double* out_loss, float* out_tangents, drt_hip_stats* stats)
{
    return render_tangents_common(ctx, cam, rp, n_dirs, param_tangents, target_rgb, residual_rgb, out_rgb, out_A, out_b, out_loss, out_tangents, stats, true);
}

} // extern "C"

// ---- one frame under several parameter sets in one trace: up to DRT_HIP_MAX_PARAM_SETS of them, or up to DRT_HIP_MAX_SETS_ALONG with a
// direction each -- value, slope and Gauss-Newton curvature of the loss per set ----
// the three forms: who is asking, the most sets it takes, and its own words where the forms' refusals differ
struct SetsForm {
    bool along;
    PathFormCaller me;
    int most;
    const char *outside, *null_input, *no_output, *needs_target;
    bool grad = false;          // drt_hip_render_param_sets_grad: reverse mode -- a seed image per set in, a summed gradient per set out, no images
    bool cross = false;         // drt_hip_render_param_sets_cross: every set's second moments too -- the unbiased loss, what was subtracted, the variance image
};
static const SetsForm plain_sets = {false,
                                    {"param sets", "render the shards on plain contexts", "a forward render", DRT_PATH_LDS_PARAMS,
                                     "more parameters than the path kernels stage (136)"},
                                    DRT_HIP_MAX_PARAM_SETS, "n_sets outside 1 ... DRT_HIP_MAX_PARAM_SETS = 8", "NULL param_sets",
                                    "no output requested (out_images and out_loss are both NULL)", "out_loss needs target_rgb"};
static const SetsForm sets_along = {true,
                                    {"param sets along", "render the shards on plain contexts", "a forward render", DRT_PATH_LDS_PARAMS,
                                     "more parameters than the path kernels stage (136)"},
                                    DRT_HIP_MAX_SETS_ALONG, "n_sets outside 1 ... DRT_HIP_MAX_SETS_ALONG = 4", "NULL param_sets or param_tangents",
                                    "no output requested (out_images, out_tangents, out_loss, out_dloss and out_curv are all NULL)",
                                    "out_loss and out_dloss need target_rgb"};
static const SetsForm sets_grad = {false,
                                   {"param sets grad", "render the shards on plain contexts", "the biased operator's summed gradients", DRT_PATH_LDS_PARAMS,
                                    "more parameters than the path kernels stage (136)"},
                                   DRT_HIP_MAX_SETS_GRAD, "n_sets outside 1 ... DRT_HIP_MAX_SETS_GRAD = 8", "NULL param_sets or out_param_grads",
                                   "", "", true};
static const SetsForm sets_cross = {false,
                                    {"param sets cross", "render the shards on plain contexts", "a forward render", DRT_PATH_LDS_PARAMS,
                                     "more parameters than the path kernels stage (136)"},
                                    DRT_HIP_MAX_SETS_CROSS, "n_sets outside 1 ... DRT_HIP_MAX_SETS_CROSS = 8", "NULL param_sets",
                                    "NULL out_loss", "NULL target_rgb", false, true};

// this shard's rows of n_sets images, from `from` bytes into ctx->neq_jac to the caller's buffer: a copy per band (the render has waited
// for its stream)
static int fetch_set_images(drt_hip_ctx* ctx, const drt_camera_desc* cam, int n_sets, void* out, size_t from, size_t el)
{
    const RenderJob& j = ctx->job;
    const size_t row = (size_t)cam->width * 3 * el, img = (size_t)cam->height * row;
    hipError_t e = hipSuccess;
    for (size_t k = 0; k < (size_t)n_sets; ++k)
        for_each_band(cam->height, j.band, j.n_shards, j.shard, [&](int y0, int y1) {
            const size_t at = k * img + (size_t)y0 * row;
            if (e == hipSuccess)
                e = hipMemcpy((uint8_t*)out + at, (const uint8_t*)ctx->neq_jac.p + from + at, (size_t)(y1 - y0) * row, hipMemcpyDeviceToHost);
        });
    HIPCHK(ctx, e);
    return DRT_OK;
}

// the one call behind the six entry points.  The plain form has no param_tangents, out_tangents, out_dloss and out_curv; the form with
// directions has no out_rgb; the gradient form has adjoints_rgb and out_param_grads and nothing else.  `wide`: the images are double (host
// buffers only).  The form with second moments has target_rgb and out_loss always, out_bias and out_variance, and no out_rgb
static int render_sets_common(drt_hip_ctx* ctx, const SetsForm& form, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_sets,
                              const double* param_sets, const double* param_tangents, const float* target_rgb, void* out_images, void* out_tangents,
                              bool wide, double* out_loss, double* out_dloss, double* out_curv, float* out_rgb, drt_hip_stats* stats,
                              const float* adjoints_rgb = nullptr, double* out_param_grads = nullptr, double* out_bias = nullptr,
                              float* out_variance = nullptr)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    const PathFormCaller& me = form.me;
    if (wide && rp && (rp->flags & DRT_RENDER_DEVICE_OUT))
        return refuse(ctx, me, DRT_ERR_INVALID, "the double images come through host buffers only (no DRT_RENDER_DEVICE_OUT)");
    int rc;
    if ((rc = refuse_before(ctx, cam, rp, me)) != DRT_OK) return rc;
    if (n_sets < 1 || n_sets > form.most)
        return refuse(ctx, me, DRT_ERR_INVALID, form.outside);
    if (!param_sets || (form.along && !param_tangents) || (form.grad && !out_param_grads))
        return refuse(ctx, me, DRT_ERR_INVALID, form.null_input);
    if (!form.grad && !out_images && !out_tangents && !out_loss && !out_dloss && !out_curv)
        return refuse(ctx, me, DRT_ERR_INVALID, form.no_output);
    if ((out_loss || out_dloss || form.cross) && !target_rgb)
        return refuse(ctx, me, DRT_ERR_INVALID, form.needs_target);
    if (form.cross && !out_loss)
        return refuse(ctx, me, DRT_ERR_INVALID, form.no_output);
    if (form.cross && rp->spp < 2)
        return refuse(ctx, me, DRT_ERR_INVALID, "spp < 2 (a product of two different samples of a pixel needs two)");
    if (!form.grad && (rp->flags & DRT_RENDER_BACKWARD))
        return refuse(ctx, me, DRT_ERR_INVALID, "a forward render: no DRT_RENDER_BACKWARD");
    for (size_t i = 0; i < (size_t)n_sets * (size_t)ctx->n_user_params * 3; ++i) {
        if (!std::isfinite(param_sets[i]))
            return refuse(ctx, me, DRT_ERR_INVALID, "a set holds a value that is not finite");
        if (form.along && !std::isfinite(param_tangents[i]))
            return refuse(ctx, me, DRT_ERR_INVALID, "a direction holds a value that is not finite");
    }
    if (!(rp->flags & DRT_RENDER_DEVICE_OUT) && target_rgb)
        for (size_t i = 0; i < (size_t)cam->width * (size_t)cam->height * 3; ++i)
            if (!std::isfinite(target_rgb[i]))
                return refuse(ctx, me, DRT_ERR_INVALID, "the target image holds a value that is not finite");
    if (!(rp->flags & DRT_RENDER_DEVICE_OUT) && adjoints_rgb)
        for (size_t i = 0; i < (size_t)n_sets * (size_t)cam->width * (size_t)cam->height * 3; ++i)
            if (!std::isfinite(adjoints_rgb[i]))
                return refuse(ctx, me, DRT_ERR_INVALID, "an adjoint image holds a value that is not finite");
    if ((rc = refuse_after(ctx, cam, rp, me)) != DRT_OK) return rc;
    // (the plain image is the kernel's last set, the context's own parameters: one set more)
    const int n_int = n_sets + (out_rgb ? 1 : 0);
    if (n_int > DRT_HIP_MAX_PARAM_SETS)
        return refuse(ctx, me, DRT_ERR_UNSUPPORTED, "out_rgb beside 8 sets (the plain image takes one of the kernel's eight: drt_hip_render gives it)");
    // (sets at and above n_sets, up to the kernel's width, are the context's own parameters -- the last one is the plain image's --, with a
    //  zero direction; a mirror's internal constant keeps the scene's value and a zero tangent in every set)
    const int K = n_int <= 2 ? 2 : (n_int <= 4 ? 4 : 8);
    if (form.grad) {
        // the form's own limit: a wave's fp64 table holds the K sets' rows, 3 per parameter that requires a gradient, once at least
        const int rows = K * std::max(1, ctx->n_grad_slots) * 3;
        if (rows > DRT_GEN_TABLE)
            return refuse(ctx, me, DRT_ERR_UNSUPPORTED, "the kernel's width of " + std::to_string(K) + " sets x " + std::to_string(std::max(1, ctx->n_grad_slots) * 3) +
                                                        " gradient rows = " + std::to_string(rows) + " rows, more than the " + std::to_string(DRT_GEN_TABLE) +
                                                        " elements of a wave's gradient table (fewer sets per call, or fewer parameters that require a gradient)");
    }
    if ((rc = form.along ? stage_rows(ctx, rp, param_sets, 2 * n_sets, 2 * K, RowPad::own_even, param_tangents)
                         : stage_rows(ctx, rp, param_sets, n_sets, K, RowPad::own)) != DRT_OK) return rc;
    const bool dev = (rp->flags & DRT_RENDER_DEVICE_OUT) != 0;
    const size_t npix = (size_t)cam->width * (size_t)cam->height;
    // the caller's images: device pointers as they are; host buffers through buffers of the context's own
    ParamSetsRequest q;
    q.n_sets = n_sets;
    q.width = K;
    q.along = form.along;
    q.grad = form.grad;
    q.cross = form.cross;
    const size_t el = wide ? sizeof(double) : sizeof(float), n_img = (size_t)n_sets * npix * 3 * el, ns3 = (size_t)n_sets * 3;
    const size_t n_grads = (size_t)n_sets * (size_t)ctx->n_user_params * 3;
    if (form.grad) {
        // the seeds in, the gradients out: device pointers as they are; host buffers through buffers of the context's own
        HIPCHK(ctx, hipSetDevice(ctx->device));
        q.d_adjoints = adjoints_rgb;
        q.d_grads = out_param_grads;
        if (!dev) {
            if (adjoints_rgb) {
                if ((rc = ensure(ctx, ctx->neq_jac, (size_t)n_sets * npix * 3 * sizeof(float))) != DRT_OK) return rc;
                HIPCHK(ctx, hipMemcpyAsync(ctx->neq_jac.p, adjoints_rgb, (size_t)n_sets * npix * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
                q.d_adjoints = (const float*)ctx->neq_jac.p;
            }
            if ((rc = ensure(ctx, ctx->neq_out, (n_grads ? n_grads : 1) * sizeof(double))) != DRT_OK) return rc;
            q.d_grads = (double*)ctx->neq_out.p;
        }
        // (a shard without rows launches nothing: its sums are zero)
        if (n_grads) HIPCHK(ctx, hipMemsetAsync(q.d_grads, 0, n_grads * sizeof(double), ctx->stream));
    } else
    if (dev) {
        q.d_target = target_rgb;
        q.d_images = (float*)out_images;
        q.d_tangents = (float*)out_tangents;
        q.d_loss = out_loss;
        q.d_dloss = out_dloss;
        q.d_curv = out_curv;
        q.d_bias = out_bias;
        q.d_variance = out_variance;
    } else {
        if (target_rgb) {
            if ((rc = ensure(ctx, ctx->neq_in, npix * 3 * sizeof(float))) != DRT_OK) return rc;
            HIPCHK(ctx, hipMemcpyAsync(ctx->neq_in.p, target_rgb, npix * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
            q.d_target = (const float*)ctx->neq_in.p;
        }
        if (out_images || out_tangents || out_variance) {
            // (the images, then the derivative images / the variance images)
            if ((rc = ensure(ctx, ctx->neq_jac, (form.along || form.cross ? 2 : 1) * n_img)) != DRT_OK) return rc;
            uint8_t* base = (uint8_t*)ctx->neq_jac.p;
            if (out_images && wide) q.d_images64 = (double*)base;
            if (out_images && !wide) q.d_images = (float*)base;
            if (out_tangents && wide) q.d_tangents64 = (double*)(base + n_img);
            if (out_tangents && !wide) q.d_tangents = (float*)(base + n_img);
            if (out_variance) q.d_variance = (float*)(base + n_img);
        }
        if (out_loss || out_dloss || out_curv) {
            if ((rc = ensure(ctx, ctx->neq_out, (size_t)(form.along ? DRT_SETS_ALONG_VALUES : 2 * DRT_SETS_VALUES) * sizeof(double))) != DRT_OK) return rc;
            double* sums = (double*)ctx->neq_out.p;
            if (out_loss) q.d_loss = sums;
            if (out_bias) q.d_bias = sums + ns3;
            if (out_dloss) q.d_dloss = sums + ns3;
            if (out_curv) q.d_curv = sums + 2 * ns3;
        }
    }
    // (a shard without rows launches nothing: its sums are zero)
    for (double* sum : {q.d_loss, q.d_dloss, q.d_curv, q.d_bias})
        if (sum) HIPCHK(ctx, hipMemsetAsync(sum, 0, ns3 * sizeof(double), ctx->stream));
    TangentRequest req;
    req.kind = TangentRequest::Kind::param_sets;
    req.d_params = ctx->tangent.p;
    req.sets = &q;
    // (the gradient form: DRT_RENDER_BACKWARD is implied -- the pipeline below is told a forward render: this form's seeds and sums go their own way)
    drt_render_params r = *rp;
    r.flags &= ~(uint32_t)DRT_RENDER_BACKWARD;
    if ((rc = render_common(ctx, cam, &r, nullptr, out_rgb, nullptr, stats, -1, nullptr, &req)) != DRT_OK)
        return rc;
    if (dev)
        return DRT_OK;
    // host buffers: the render has waited for its stream; the sums, and the images' rows of this shard
    if (form.grad && n_grads) HIPCHK(ctx, hipMemcpy(out_param_grads, q.d_grads, n_grads * sizeof(double), hipMemcpyDeviceToHost));
    if (out_loss) HIPCHK(ctx, hipMemcpy(out_loss, q.d_loss, ns3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_dloss) HIPCHK(ctx, hipMemcpy(out_dloss, q.d_dloss, ns3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_curv) HIPCHK(ctx, hipMemcpy(out_curv, q.d_curv, ns3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_images && (rc = fetch_set_images(ctx, cam, n_sets, out_images, 0, el)) != DRT_OK) return rc;
    if (out_tangents && (rc = fetch_set_images(ctx, cam, n_sets, out_tangents, n_img, el)) != DRT_OK) return rc;
    if (out_bias) HIPCHK(ctx, hipMemcpy(out_bias, q.d_bias, ns3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_variance && (rc = fetch_set_images(ctx, cam, n_sets, out_variance, n_img, el)) != DRT_OK) return rc;
    return DRT_OK;
}

extern "C" {

int drt_hip_render_param_sets(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_sets,
                              const double* param_sets, const float* target_rgb, float* out_images, double* out_loss, float* out_rgb,
                              drt_hip_stats* stats)
{
    return render_sets_common(ctx, plain_sets, cam, rp, n_sets, param_sets, nullptr, target_rgb, out_images, nullptr, false, out_loss, nullptr, nullptr,
                              out_rgb, stats);
}

int drt_hip_render_param_sets_double(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_sets,
                                     const double* param_sets, const float* target_rgb, double* out_images, double* out_loss, float* out_rgb,
                                     drt_hip_stats* stats)
{
    return render_sets_common(ctx, plain_sets, cam, rp, n_sets, param_sets, nullptr, target_rgb, out_images, nullptr, true, out_loss, nullptr, nullptr,
                              out_rgb, stats);
}

int drt_hip_render_param_sets_along(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_sets,
                                    const double* param_sets, const double* param_tangents, const float* target_rgb, float* out_images,
                                    float* out_tangents, double* out_loss, double* out_dloss, double* out_curv, drt_hip_stats* stats)
{
    return render_sets_common(ctx, sets_along, cam, rp, n_sets, param_sets, param_tangents, target_rgb, out_images, out_tangents, false, out_loss,
                              out_dloss, out_curv, nullptr, stats);
}

int drt_hip_render_param_sets_along_double(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_sets,
                                           const double* param_sets, const double* param_tangents, const float* target_rgb, double* out_images,
                                           double* out_tangents, double* out_loss, double* out_dloss, double* out_curv, drt_hip_stats* stats)
{
    return render_sets_common(ctx, sets_along, cam, rp, n_sets, param_sets, param_tangents, target_rgb, out_images, out_tangents, true, out_loss,
                              out_dloss, out_curv, nullptr, stats);
}

int drt_hip_render_param_sets_grad(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_sets,
                                   const double* param_sets, const float* adjoints_rgb, double* out_param_grads, drt_hip_stats* stats)
{
    return render_sets_common(ctx, sets_grad, cam, rp, n_sets, param_sets, nullptr, nullptr, nullptr, nullptr, false, nullptr, nullptr, nullptr, nullptr,
                              stats, adjoints_rgb, out_param_grads);
}

int drt_hip_render_param_sets_cross(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_sets,
                                    const double* param_sets, const float* target_rgb, float* out_images, double* out_loss, double* out_bias,
                                    float* out_variance, drt_hip_stats* stats)
{
    return render_sets_common(ctx, sets_cross, cam, rp, n_sets, param_sets, nullptr, target_rgb, out_images, nullptr, false, out_loss, nullptr, nullptr,
                              nullptr, stats, nullptr, nullptr, out_bias, out_variance);
}

} // extern "C"

// ---- one scene from several cameras in one trace (k_path_views, drt_path.h) ----------------------------------------------------------
// The call's pinned block: stage_rows' two pinned copies and their events, used the same way (this call has no rows behind the kernel's
// `params`, so the buffers are free for it).  [the views' table | `extra` bytes of the caller's]: the table goes to ctx->tangent.p in stream
// order; -> the block (the extra bytes start 16-byte aligned behind the table: views_extra_offset)
static size_t views_extra_offset(int n_views) { return ((size_t)n_views * sizeof(PathView) + 15) & ~(size_t)15; }
static int stage_views(drt_hip_ctx* ctx, const drt_camera_desc* cams, int n_views, const drt_render_params* rp, const uint32_t* seeds, size_t extra,
                       uint8_t** block)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int hb = (int)(ctx->tangent_calls++ & 1);
    const size_t bytes = (size_t)n_views * sizeof(PathView), need = (views_extra_offset(n_views) + extra + sizeof(double) - 1) / sizeof(double);
    if (!ctx->ev_tangent[hb])
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_tangent[hb], hipEventDisableTiming));
    else
        HIPCHK(ctx, hipEventSynchronize(ctx->ev_tangent[hb]));
    if (ctx->h_tangent_cap[hb] < need) {
        if (ctx->h_tangent[hb])
            (void)hipHostFree(ctx->h_tangent[hb]);
        ctx->h_tangent[hb] = nullptr;
        ctx->h_tangent_cap[hb] = 0;
        HIPCHK(ctx, hipHostMalloc((void**)&ctx->h_tangent[hb], need * sizeof(double)));
        ctx->h_tangent_cap[hb] = need;
    }
    PathView* tab = reinterpret_cast<PathView*>(ctx->h_tangent[hb]);
    for (int v = 0; v < n_views; ++v)
        fill_path_view(tab[v], cams[v], seeds ? seeds[v] : rp->seed);
    int rc;
    if ((rc = ensure(ctx, ctx->tangent, bytes)) != DRT_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->tangent.p, tab, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev_tangent[hb], ctx->stream));
    *block = reinterpret_cast<uint8_t*>(ctx->h_tangent[hb]);
    return DRT_OK;
}

extern "C" {

int drt_hip_render_views(drt_hip_ctx* ctx, const drt_camera_desc* cams, int32_t n_views, const drt_render_params* rp, const uint32_t* seeds,
                         const float* adjoints_rgb, float* out_images, double* out_param_grad, double* out_view_grads, drt_hip_stats* stats)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    static const PathFormCaller me = {"views", "render the shards on plain contexts", "the biased operator", DRT_PATH_LDS_PARAMS,
                                      "more parameters than the path kernels stage (136)"};
    int rc;
    if ((rc = refuse_before(ctx, cams, rp, me)) != DRT_OK) return rc;
    if (n_views < 1 || n_views > DRT_HIP_MAX_VIEWS)
        return refuse(ctx, me, DRT_ERR_INVALID, "n_views outside 1 ... DRT_HIP_MAX_VIEWS = 64");
    for (int v = 1; v < n_views; ++v)
        if (cams[v].width != cams[0].width || cams[v].height != cams[0].height)
            return refuse(ctx, me, DRT_ERR_INVALID, "the cameras differ in width or height (all views share one size)");
    if (!out_images && !out_param_grad && !out_view_grads)
        return refuse(ctx, me, DRT_ERR_INVALID, "no output requested (out_images, out_param_grad and out_view_grads are all NULL)");
    const bool backward = (out_param_grad || out_view_grads);
    if (backward && !(rp->flags & DRT_RENDER_BACKWARD))
        return refuse(ctx, me, DRT_ERR_INVALID, "out_param_grad and out_view_grads need DRT_RENDER_BACKWARD");
    const bool dev = (rp->flags & DRT_RENDER_DEVICE_OUT) != 0;
    const size_t npix = (size_t)cams[0].width * (size_t)cams[0].height;
    if (!dev && adjoints_rgb)
        for (size_t i = 0; i < (size_t)n_views * npix * 3; ++i)
            if (!std::isfinite(adjoints_rgb[i]))
                return refuse(ctx, me, DRT_ERR_INVALID, "an adjoint image holds a value that is not finite");
    if ((rc = refuse_after(ctx, cams, rp, me)) != DRT_OK) return rc;
    if ((uint64_t)n_views * npix * (uint64_t)(rp->spp > 0 ? rp->spp : 1) > 0x7FFFFFFFull)
        return refuse(ctx, me, DRT_ERR_UNSUPPORTED, "more than 2^31 camera samples over all views (they render in one launch)");
    // Host buffers: everything crosses in the call's pinned block, [table | gradients (the views', then their sum) | images | adjoint images] --
    // the finishing kernel stores images and sums straight into it (no device copy, no copy launch behind it, as a synchronous drt_hip_render
    // does), and the path kernel reads its seeds from it where they are small (one 12-byte load per lane: render_impl's rule), from a copy in
    // device memory else.  Device pointers: the table alone
    const size_t n_img = (size_t)n_views * npix * 3 * sizeof(float), ng = (size_t)ctx->n_user_params * 3;
    const bool host_adj = !dev && backward && adjoints_rgb;
    const size_t grad_bytes = (((size_t)(n_views + 1) * ng + 1) * sizeof(double) + 15) & ~(size_t)15, img_bytes = (n_img + 15) & ~(size_t)15;
    const size_t off_grad = views_extra_offset(n_views), off_img = off_grad + (backward ? grad_bytes : 0), off_adj = off_img + (out_images ? img_bytes : 0);
    uint8_t* block = nullptr;
    if ((rc = stage_views(ctx, cams, n_views, rp, seeds, dev ? 0 : off_adj + (host_adj ? n_img : 0) - off_grad, &block)) != DRT_OK) return rc;
    ViewsRequest q;
    q.n_views = n_views;
    q.backward = backward;
    q.d_table = ctx->tangent.p;
    if (dev) {
        q.d_adjoints = backward ? adjoints_rgb : nullptr;
        q.d_images = out_images;
        q.d_view_grads = out_view_grads;
        q.d_grad = out_param_grad;
        // (a shard without rows launches nothing: its sums are zero)
        if (rp->n_shards > 1) {
            if (q.d_view_grads && ng) HIPCHK(ctx, hipMemsetAsync(q.d_view_grads, 0, (size_t)n_views * ng * sizeof(double), ctx->stream));
            if (q.d_grad && ng) HIPCHK(ctx, hipMemsetAsync(q.d_grad, 0, ng * sizeof(double), ctx->stream));
        }
    } else {
        if (host_adj) {
            memcpy(block + off_adj, adjoints_rgb, n_img);
            q.d_adjoints = (const float*)(block + off_adj);
            if (n_img > ((size_t)1 << 20)) {
                if ((rc = ensure(ctx, ctx->neq_in, n_img)) != DRT_OK) return rc;
                HIPCHK(ctx, hipMemcpyAsync(ctx->neq_in.p, block + off_adj, n_img, hipMemcpyHostToDevice, ctx->stream));
                q.d_adjoints = (const float*)ctx->neq_in.p;
            }
        }
        if (out_images)
            q.d_images = (float*)(block + off_img);
        if (backward) {
            q.d_view_grads = (double*)(block + off_grad);
            q.d_grad = q.d_view_grads + (size_t)n_views * ng;
            memset(q.d_view_grads, 0, (size_t)(n_views + 1) * ng * sizeof(double));      // (a shard without rows launches nothing: its sums are zero)
        }
    }
    TangentRequest req;
    req.kind = TangentRequest::Kind::views;
    req.views = &q;
    // (the pipeline below is told a forward render of the first camera: this form's seeds, images and sums go their own way)
    drt_render_params r = *rp;
    r.flags &= ~(uint32_t)DRT_RENDER_BACKWARD;
    if ((rc = render_common(ctx, &cams[0], &r, nullptr, nullptr, nullptr, stats, -1, nullptr, &req)) != DRT_OK)
        return rc;
    if (dev)
        return DRT_OK;
    // host buffers: the render has waited for its stream; the sums, and the images' rows of this shard
    if (out_view_grads && ng) memcpy(out_view_grads, q.d_view_grads, (size_t)n_views * ng * sizeof(double));
    if (out_param_grad && ng) memcpy(out_param_grad, q.d_grad, ng * sizeof(double));
    if (out_images) {
        const RenderJob& j = ctx->job;
        const size_t row = (size_t)cams[0].width * 3 * sizeof(float), img = (size_t)cams[0].height * row;
        for (size_t v = 0; v < (size_t)n_views; ++v)
            for_each_band(cams[0].height, j.band, j.n_shards, j.shard, [&](int y0, int y1) {
                const size_t at = v * img + (size_t)y0 * row;
                memcpy((uint8_t*)out_images + at, block + off_img + at, (size_t)(y1 - y0) * row);
            });
    }
    return DRT_OK;
}

} // extern "C"

// ---- a caller's batch of pixels from several cameras in one trace (k_path_pixels, drt_path.h) -----------------------------------------
// The call's pinned block, stage_views' buffers used the same way: [head | the views' records | the pixel lists], then `extra` bytes of the
// caller's.  The records' cameras and seeds and the lists are filled here; the views' places in the grid need the plan's sample ranges, so
// path_batch adds them and copies [head | records | lists] to ctx->tangent.p in stream order (the caller records the block's event behind it)
static size_t pixels_list_offset(int n_views) { return (sizeof(PixelsHead) + (size_t)n_views * sizeof(PixelView) + 15) & ~(size_t)15; }
static int stage_pixels(drt_hip_ctx* ctx, const drt_camera_desc* cams, int n_views, const drt_render_params* rp, const uint32_t* seeds,
                        const uint32_t* pixels, size_t n_entries, size_t copy_bytes, size_t extra, int* which, uint8_t** block)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int hb = (int)(ctx->tangent_calls++ & 1);
    const size_t need = (copy_bytes + extra + sizeof(double) - 1) / sizeof(double);
    if (!ctx->ev_tangent[hb])
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_tangent[hb], hipEventDisableTiming));
    else
        HIPCHK(ctx, hipEventSynchronize(ctx->ev_tangent[hb]));
    if (ctx->h_tangent_cap[hb] < need) {
        if (ctx->h_tangent[hb])
            (void)hipHostFree(ctx->h_tangent[hb]);
        ctx->h_tangent[hb] = nullptr;
        ctx->h_tangent_cap[hb] = 0;
        HIPCHK(ctx, hipHostMalloc((void**)&ctx->h_tangent[hb], need * sizeof(double)));
        ctx->h_tangent_cap[hb] = need;
    }
    uint8_t* b = reinterpret_cast<uint8_t*>(ctx->h_tangent[hb]);
    PixelView* pv = const_cast<PixelView*>(pixel_views(reinterpret_cast<PixelsHead*>(b)));
    for (int v = 0; v < n_views; ++v) {
        memset(&pv[v], 0, sizeof pv[v]);
        fill_path_view(pv[v].cam, cams[v], seeds ? seeds[v] : rp->seed);
    }
    memcpy(b + pixels_list_offset(n_views), pixels, n_entries * sizeof(uint32_t));
    int rc;
    if ((rc = ensure(ctx, ctx->tangent, copy_bytes)) != DRT_OK) return rc;
    *which = hb;
    *block = b;
    return DRT_OK;
}

extern "C" {

int drt_hip_render_pixels(drt_hip_ctx* ctx, const drt_camera_desc* cams, int32_t n_views, const drt_render_params* rp, const uint32_t* seeds,
                          const int32_t* counts, const uint32_t* pixels, const float* adjoints_rgb, float* out_rgb, double* out_param_grad,
                          double* out_view_grads, drt_hip_stats* stats)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    static_assert(DRT_PIXELS_MAX_VIEWS == DRT_HIP_MAX_VIEWS && DRT_PIXELS_WAVE == DRT_WAVE && DRT_PIXELS_BLOCK_WAVES * DRT_WAVE == DRT_BLOCK,
                  "drt_pixels.h packs for this grid");
    static_assert(sizeof(PixelsHead) == DRT_HIP_MAX_VIEWS * sizeof(uint32_t) && sizeof(PixelView) % 8 == 0, "the table's layout");
    static const PathFormCaller me = {"pixels", "render the lists on plain contexts", "the biased operator", DRT_PATH_LDS_PARAMS,
                                      "more parameters than the path kernels stage (136)"};
    int rc;
    if ((rc = refuse_before(ctx, cams, rp, me)) != DRT_OK) return rc;
    if (n_views < 1 || n_views > DRT_HIP_MAX_VIEWS)
        return refuse(ctx, me, DRT_ERR_INVALID, pixels_refusal_text(DRT_PIXELS_N_VIEWS));
    for (int v = 1; v < n_views; ++v)
        if (cams[v].width != cams[0].width || cams[v].height != cams[0].height)
            return refuse(ctx, me, DRT_ERR_INVALID, "the cameras differ in width or height (all views share one size)");
    if (rp->n_shards > 1)
        return refuse(ctx, me, DRT_ERR_INVALID, "not with n_shards > 1 (a list is the caller's own split of the work)");
    if (!out_rgb && !out_param_grad && !out_view_grads)
        return refuse(ctx, me, DRT_ERR_INVALID, "no output requested (out_rgb, out_param_grad and out_view_grads are all NULL)");
    const bool backward = (out_param_grad || out_view_grads);
    if (backward && !(rp->flags & DRT_RENDER_BACKWARD))
        return refuse(ctx, me, DRT_ERR_INVALID, "out_param_grad and out_view_grads need DRT_RENDER_BACKWARD");
    // the lists (drt_pixels.h): refused before anything is enqueued
    uint64_t n_entries = 0;
    const int why = pixels_check(counts, n_views, pixels, (uint64_t)cams[0].width * (uint64_t)cams[0].height, (uint64_t)(rp->spp > 0 ? rp->spp : 1), &n_entries);
    if (why != DRT_PIXELS_OK && why != DRT_PIXELS_TOO_MANY)
        return refuse(ctx, me, DRT_ERR_INVALID, pixels_refusal_text(why));
    const bool dev = (rp->flags & DRT_RENDER_DEVICE_OUT) != 0;
    if (why == DRT_PIXELS_OK && !dev && adjoints_rgb)
        for (size_t i = 0; i < (size_t)n_entries * 3; ++i)
            if (!std::isfinite(adjoints_rgb[i]))
                return refuse(ctx, me, DRT_ERR_INVALID, "an adjoint holds a value that is not finite");
    if ((rc = refuse_after(ctx, cams, rp, me)) != DRT_OK) return rc;
    if (why == DRT_PIXELS_TOO_MANY)
        return refuse(ctx, me, DRT_ERR_UNSUPPORTED, pixels_refusal_text(why));
    // Host buffers: everything crosses in the call's pinned block, [table | pixels | gradients (the views', then their sum) | radiance |
    // adjoints] -- the finishing kernel stores radiance and sums straight into it, and the path kernel reads its seeds from it where they
    // are small (one 12-byte load per lane: render_impl's rule), from a copy in device memory else.  Device pointers: [table | pixels] alone
    const size_t n_rgb = (size_t)n_entries * 3 * sizeof(float), ng = (size_t)ctx->n_user_params * 3;
    const bool host_adj = !dev && backward && adjoints_rgb;
    const size_t off_pix = pixels_list_offset(n_views), copy_bytes = off_pix + (size_t)n_entries * sizeof(uint32_t);
    const size_t grad_bytes = (((size_t)(n_views + 1) * ng + 1) * sizeof(double) + 15) & ~(size_t)15, rgb_bytes = (n_rgb + 15) & ~(size_t)15;
    const size_t off_grad = (copy_bytes + 15) & ~(size_t)15, off_rgb = off_grad + (backward ? grad_bytes : 0), off_adj = off_rgb + (out_rgb ? rgb_bytes : 0);
    uint8_t* block = nullptr;
    int hb = 0;
    if ((rc = stage_pixels(ctx, cams, n_views, rp, seeds, pixels, (size_t)n_entries, copy_bytes,
                           dev ? 0 : off_adj + (host_adj ? n_rgb : 0) - copy_bytes, &hb, &block)) != DRT_OK) return rc;
    PixelsRequest q;
    q.n_views = n_views;
    q.backward = backward;
    q.counts = counts;
    q.n_entries = n_entries;
    q.h_table = block;
    q.d_table = ctx->tangent.p;
    q.table_bytes = copy_bytes;
    q.d_pixels = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(ctx->tangent.p) + off_pix);
    if (dev) {
        q.d_adjoints = backward ? adjoints_rgb : nullptr;
        q.d_rgb = out_rgb;
        q.d_view_grads = out_view_grads;
        q.d_grad = out_param_grad;
    } else {
        if (host_adj) {
            memcpy(block + off_adj, adjoints_rgb, n_rgb);
            q.d_adjoints = (const float*)(block + off_adj);
            if (n_rgb > ((size_t)1 << 20)) {
                if ((rc = ensure(ctx, ctx->neq_in, n_rgb)) != DRT_OK) return rc;
                HIPCHK(ctx, hipMemcpyAsync(ctx->neq_in.p, block + off_adj, n_rgb, hipMemcpyHostToDevice, ctx->stream));
                q.d_adjoints = (const float*)ctx->neq_in.p;
            }
        }
        if (out_rgb)
            q.d_rgb = (float*)(block + off_rgb);
        if (backward) {
            q.d_view_grads = (double*)(block + off_grad);
            q.d_grad = q.d_view_grads + (size_t)n_views * ng;
        }
    }
    TangentRequest req;
    req.kind = TangentRequest::Kind::pixels;
    req.pixels = &q;
    // (the pipeline below is told a forward render of the first camera's whole frame -- the plan's sample ranges are that frame's --: this
    //  form's seeds, radiance and sums go their own way)
    drt_render_params r = *rp;
    r.flags &= ~(uint32_t)DRT_RENDER_BACKWARD;
    rc = render_common(ctx, &cams[0], &r, nullptr, nullptr, nullptr, stats, -1, nullptr, &req);
    // (the block is free again once the table's copy -- and, host buffers, the adjoints' -- has been made)
    (void)hipEventRecord(ctx->ev_tangent[hb], ctx->stream);
    if (rc != DRT_OK || dev)
        return rc;
    // host buffers: the render has waited for its stream
    if (out_view_grads && ng) memcpy(out_view_grads, q.d_view_grads, (size_t)n_views * ng * sizeof(double));
    if (out_param_grad && ng) memcpy(out_param_grad, q.d_grad, ng * sizeof(double));
    if (out_rgb) memcpy(out_rgb, block + off_rgb, n_rgb);
    return DRT_OK;
}

// ---- the per-sample loss from the caller's own source (drt_loss.h) ---------------------------------------------------
// "drt_sample_loss.h" as hiprtc sees it: the one function, the caller's text its body -- and nothing else of the caller's: the header, and
// with it the compile cache's key, is the source alone.  The loss's name is for messages, reduced to letters, digits and [ _.-].
static std::string sample_loss_header(const char* src)
{
    return std::string("template <typename R>\n"
                       "__device__ inline void sample_loss(const R* q, V3<R> L, V3<R> t, R& value, V3<R>& grad)\n"
                       "{\n") + src + "\n}\n";
}
static std::string sample_loss_name(const char* name)
{
    std::string clean;
    for (const char* c = name ? name : ""; *c && clean.size() < 64; ++c)
        clean += (isalnum((unsigned char)*c) || *c == '_' || *c == '.' || *c == '-' || *c == ' ') ? *c : '_';
    return clean;
}
// the squared error, DRT_RENDER_LOSS_L2's seed 2 (L - t) with its value
static const char* const sample_loss_l2_src = "    const V3<R> d = L - t;\n    value = dot(d, d);\n    grad = mk<R>(R(2) * d.x, R(2) * d.y, R(2) * d.z);";

int drt_hip_set_sample_loss(drt_hip_ctx* ctx, const drt_sample_loss_desc* loss)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    if (!ctx->members.empty())
        return fail(ctx, DRT_ERR_UNSUPPORTED, "set_sample_loss: no sample loss on a group context");
    if (loss && !loss->loss_src)
        return fail(ctx, DRT_ERR_INVALID, "set_sample_loss: a sample loss needs its source (loss_src)");
    for (int k = 0; loss && k < DRT_MAX_LOSS_VALUES; ++k)
        if (!std::isfinite(loss->values[k]))
            return fail(ctx, DRT_ERR_INVALID, "set_sample_loss: the sample loss holds a value that is not finite");
    ctx->loss_header = loss ? sample_loss_header(loss->loss_src) : std::string();
    ctx->loss_name = loss ? sample_loss_name(loss->name) : std::string();
    for (int k = 0; k < DRT_MAX_LOSS_VALUES; ++k)
        ctx->loss_values[k] = loss ? loss->values[k] : 0.0;
    return DRT_OK;
}

int drt_hip_render_sample_loss(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, const float* target_rgb,
                               float* out_rgb, double* out_param_grad, double* out_loss, drt_hip_stats* stats)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    if (!ctx->members.empty())
        return fail(ctx, DRT_ERR_UNSUPPORTED, "sample loss: not on a group context (render the shards on plain contexts and add their gradients and losses)");
    if (!ctx->has_scene)
        return fail(ctx, DRT_ERR_NO_SCENE, "render before upload_scene");
    if (!cam || !rp || cam->width <= 0 || cam->height <= 0)
        return fail(ctx, DRT_ERR_INVALID, "sample loss: bad camera or render parameters");
    if (!target_rgb)
        return fail(ctx, DRT_ERR_INVALID, "sample loss: NULL target_rgb");
    if (!out_rgb && !out_param_grad && !out_loss)
        return fail(ctx, DRT_ERR_INVALID, "sample loss: nothing to return (out_rgb, out_param_grad and out_loss are all NULL)");
    if (rp->flags & (DRT_RENDER_UNBIASED | DRT_RENDER_ALLREDUCE | DRT_RENDER_ALLREDUCE_ASYNC))
        return fail(ctx, DRT_ERR_INVALID, "sample loss: not with DRT_RENDER_UNBIASED or _ALLREDUCE* (the biased operator, one context; the shards' gradients and losses add)");
    for (int i = 0; i < DRT_HIP_FRAMES_IN_FLIGHT; ++i)
        if (ctx->in_flight[i])
            return fail(ctx, DRT_ERR_INVALID, "sample loss: asynchronous frames are in flight -- drt_hip_wait for them first");
    const bool dev_out = (rp->flags & DRT_RENDER_DEVICE_OUT) != 0;
    if (!dev_out) {
        const size_t n = (size_t)cam->width * (size_t)cam->height * 3;
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(target_rgb[i]))
                return fail(ctx, DRT_ERR_INVALID, "sample loss: the target image holds a value that is not finite");
    }
    if (ctx->jit_mode <= 0)
        return fail(ctx, DRT_ERR_UNSUPPORTED, "sample loss: the loss is compiled at run time and this context may not compile (drt_hip_set_specialisation / DRT_HIP_JIT)");
    if (ctx->loss_header.empty()) {     // (the default: its header is made once)
        ctx->loss_header = sample_loss_header(sample_loss_l2_src);
        ctx->loss_name = "squared error";
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the shard's loss (a shard without rows: zero), and behind it a place for the gradients nobody asked for
    const size_t grad_bytes = (size_t)(ctx->n_user_params > 0 ? ctx->n_user_params : 1) * 3 * sizeof(double);
    int rc;
    if ((rc = ensure(ctx, ctx->loss_out, sizeof(double) + grad_bytes)) != DRT_OK) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->loss_out.p, 0, sizeof(double), ctx->stream));
    std::vector<double> grad_sink;
    double* grad_out = out_param_grad;
    if (!grad_out) {
        if (dev_out)
            grad_out = (double*)ctx->loss_out.p + 1;
        else {
            grad_sink.resize(grad_bytes / sizeof(double));
            grad_out = grad_sink.data();
        }
    }
    drt_render_params r = *rp;
    r.flags |= DRT_RENDER_BACKWARD | DRT_RENDER_LOSS_L2;      // (the target travels as DRT_RENDER_LOSS_L2's does; the seed is the context's loss's)
    ctx->sample_loss_render = true;
    rc = render_common(ctx, cam, &r, target_rgb, out_rgb, grad_out, stats, -1, nullptr);
    ctx->sample_loss_render = false;
    if (rc != DRT_OK)
        return rc;
    if (out_loss) {
        if (dev_out)
            HIPCHK(ctx, hipMemcpyAsync(out_loss, ctx->loss_out.p, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        else
            HIPCHK(ctx, hipMemcpy(out_loss, ctx->loss_out.p, sizeof(double), hipMemcpyDeviceToHost));     // (the render has waited for the stream)
    }
    return DRT_OK;
}

// ---- asynchronous host-buffer renders ---------------------------------------------------------------
// drt_hip_render returns when the results are in the caller's buffers: every frame pays a 3 MB device-to-host copy and a
// stream synchronisation with the GPU idle meanwhile (config 3: 1.13 instead of 0.86 ms per frame).  An optimisation loop
// that renders frame after frame (render.cpp:72-90 inside a gradient-descent loop) overlaps them: frame i's results travel to
// a pinned block on a second stream while frame i + 1's kernels run; drt_hip_wait hands them over.
int drt_hip_render_async(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, const float* adjoint_rgb,
                         float* out_rgb, double* out_param_grad, uint64_t* ticket)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    if (!ticket)
        return fail(ctx, DRT_ERR_INVALID, "render_async: ticket is NULL");
    *ticket = 0;
    if (!ctx->members.empty())
        return fail(ctx, DRT_ERR_UNSUPPORTED, "render_async: not on a group context");
    if (rp && (rp->flags & (DRT_RENDER_DEVICE_OUT | DRT_RENDER_TIMING)))
        return fail(ctx, DRT_ERR_INVALID, "render_async: host buffers only, no per-kernel timing (use drt_hip_render)");
    const uint64_t t = ctx->next_ticket;
    const int slot = (int)(t % DRT_HIP_FRAMES_IN_FLIGHT);
    if (ctx->in_flight[slot])
        return fail(ctx, DRT_ERR_INVALID, "render_async: four frames are in flight already -- drt_hip_wait for the oldest one first");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    {
        const int rc0 = ensure_copy_stream(ctx);
        if (rc0 != DRT_OK) return rc0;
    }
    ctx->slot = slot;
    static drt_hip_stats sink;            // (render_launch only notes that totals are wanted; drt_hip_wait fills the caller's)
    // The frame's kernels run on the context's first stream and leave image, gradients and totals in the device buffers of the
    // frame's slot; ONE copy launch on the second stream (k_frame_to_host: zero-copy stores into the pinned block -- no DMA
    // engine, no hipMemcpy) carries them across the link while the next frame's kernels run on the first; an event marks the
    // end.  Config 3, per frame: 0.84-0.87 ms against 0.834 on device pointers and 1.10 for the synchronous call.
    // (Measured before it, round 3: the same copy as hipMemcpyAsync on the second stream -- 0.85 ms under ROCm 7.2's runtime
    // but 1.3 ms, slower than the synchronous call, when the process had loaded PyTorch's bundled ROCm 7.0 runtime first, as
    // bench.py does; and everything on ONE stream, the finishing kernels storing the image straight into the pinned block
    // (DRT_HIP_ASYNC_COPY=inline, still there): 0.89-0.92 ms -- the 3 MB cross the link inside the frame's critical path.)
    const bool two_streams = !tuning().async_copy_inline;
    ctx->zero_copy_next = !two_streams;
    // (the k_path grids of consecutive frames overlap -- render_impl: path_stream --: frame t shares its stream and its set of
    //  partial sums with frame t - 2, whose finishing launch, on the context's stream, must have read them)
    ctx->overlap_next = two_streams && !(rp && (rp->flags & DRT_RENDER_SERIAL));
    ctx->stage_adjoint_next = true;
    int rc = render_launch(ctx, cam, rp, adjoint_rgb, out_rgb, out_param_grad, &sink, -1, nullptr);
    ctx->stage_adjoint_next = false;
    ctx->zero_copy_next = false;
    ctx->overlap_next = false;
    if (rc != DRT_OK)
        abort_comm_after_failure(ctx, rp);
    if (rc == DRT_OK) rc = render_reduce(ctx);
    hipStream_t done_on = ctx->stream;
    if (rc == DRT_OK && two_streams) {
        ctx->job.copy_kernel = true;
        hipError_t e = hipEventRecord(ctx->ev_rendered[slot], ctx->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->copy_stream, ctx->ev_rendered[slot], 0);
        if (e != hipSuccess) { ctx->err = std::string("render_async: ") + hipGetErrorString(e); rc = DRT_ERR_HIP; }
        done_on = ctx->copy_stream;
    }
    if (rc == DRT_OK) rc = render_collect(ctx, true, done_on);
    if (rc == DRT_OK && hipEventRecord(ctx->ev_copied[slot], done_on) != hipSuccess) {
        ctx->err = "render_async: hipEventRecord failed";
        rc = DRT_ERR_HIP;
    }
    if (rc != DRT_OK) {                   // nothing of this frame stays in flight
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(ctx->copy_stream);
        ctx->slot = 0;
        return rc;
    }
    ctx->slot_used[slot] = true;
    ctx->pending[slot] = ctx->job;
    ctx->in_flight[slot] = true;
    ctx->next_ticket = t + 1;
    ctx->slot = 0;
    *ticket = t;
    return DRT_OK;
}

int drt_hip_wait(drt_hip_ctx* ctx, uint64_t ticket, drt_hip_stats* stats)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    const int slot = (int)(ticket % DRT_HIP_FRAMES_IN_FLIGHT);
    if (ticket == 0 || ticket >= ctx->next_ticket || !ctx->in_flight[slot] || ticket + DRT_HIP_FRAMES_IN_FLIGHT < ctx->next_ticket)
        return fail(ctx, DRT_ERR_INVALID, "wait: no such frame in flight");
    ctx->slot = slot;
    ctx->job = ctx->pending[slot];
    ctx->job.stats = stats;               // (NULL: no statistics wanted)
    const int rc = render_finish(ctx, true, ctx->ev_copied[slot]);
    ctx->in_flight[slot] = false;
    ctx->slot = 0;
    return rc;
}

// ---- multi-GPU: communicators and group contexts -------------------------------------------------
static int comm_fail(drt_hip_ctx* ctx, const char* what, ncclResult_t r)
{
    if (ctx)
        ctx->err = std::string(what) + ": " + ncclGetErrorString(r);
    return DRT_ERR_COMM;
}

int drt_hip_comm_unique_id(drt_hip_unique_id* out)
{
    static_assert(sizeof(ncclUniqueId) == DRT_HIP_UNIQUE_ID_BYTES, "drt_hip_unique_id is an ncclUniqueId");
    if (!out)
        return DRT_ERR_INVALID;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess)
        return DRT_ERR_COMM;
    memcpy(out->bytes, &id, sizeof id);
    return DRT_OK;
}

int drt_hip_comm_init_rank(drt_hip_ctx* ctx, const drt_hip_unique_id* id, int rank, int n_ranks)
{
    if (!ctx || !id || n_ranks < 1 || rank < 0 || rank >= n_ranks)
        return ctx ? fail(ctx, DRT_ERR_INVALID, "comm_init_rank: bad arguments") : DRT_ERR_INVALID;
    if (!ctx->members.empty())
        return fail(ctx, DRT_ERR_INVALID, "comm_init_rank: a group context owns its communicators already");
    if (ctx->comm)
        return fail(ctx, DRT_ERR_INVALID, "comm_init_rank: the context already has a communicator");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ncclUniqueId nid;
    memcpy(&nid, id->bytes, sizeof nid);
    const ncclResult_t r = ncclCommInitRank(&ctx->comm, n_ranks, nid, rank);
    if (r != ncclSuccess) {
        ctx->comm = nullptr;
        return comm_fail(ctx, "ncclCommInitRank", r);
    }
    ctx->comm_rank = rank;
    ctx->comm_size = n_ranks;
    return DRT_OK;
}

int drt_hip_device_pci_bus_id(const drt_hip_ctx* ctx, int member, char* out, int capacity)
{
    if (!ctx || !out || capacity < 16)
        return DRT_ERR_INVALID;
    const drt_hip_ctx* c = ctx;
    if (!ctx->members.empty()) {
        if (member < 0 || member >= (int)ctx->members.size())
            return DRT_ERR_INVALID;
        c = ctx->members[(size_t)member];
    } else if (member != 0)
        return DRT_ERR_INVALID;
    out[0] = 0;
    return hipDeviceGetPCIBusId(out, capacity, c->device) == hipSuccess ? DRT_OK : DRT_ERR_HIP;
}

int drt_hip_comm_size(const drt_hip_ctx* ctx)
{
    if (!ctx)
        return 0;
    if (!ctx->members.empty())
        return ctx->members[0]->comm_size;
    return ctx->comm ? ctx->comm_size : 0;
}

int drt_hip_comm_destroy(drt_hip_ctx* ctx)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    if (ctx->comm) {
        (void)hipSetDevice(ctx->device);
        if (ctx->stream)
            (void)hipStreamSynchronize(ctx->stream);
        (void)ncclCommDestroy(ctx->comm);
        ctx->comm = nullptr;
        ctx->comm_size = 0;
    }
    return DRT_OK;
}

int drt_hip_create_group(const int* device_ids, int n_devices, drt_hip_ctx** out)
{
    if (!out)
        return DRT_ERR_INVALID;
    *out = nullptr;
    if (!device_ids || n_devices < 1 || n_devices > 64)
        return DRT_ERR_INVALID;
    drt_hip_ctx* g = new drt_hip_ctx();
    g->device = device_ids[0];
    std::vector<int> distinct;           // the devices of the communicator, in order of first appearance
    for (int i = 0; i < n_devices; ++i) {
        drt_hip_ctx* m = nullptr;
        const int rc = drt_hip_create(device_ids[i], &m);
        if (rc != DRT_OK) {
            drt_hip_destroy(g);
            return rc;
        }
        m->is_member = true;
        g->members.push_back(m);
        int lead = i;
        for (int e = 0; e < i; ++e)
            if (device_ids[e] == device_ids[i]) { lead = e; break; }
        g->leader.push_back(lead);
        if (lead == i)
            distinct.push_back(device_ids[i]);
        if (hipEventCreateWithFlags(&m->ev_done, hipEventDisableTiming) != hipSuccess) {
            drt_hip_destroy(g);
            return DRT_ERR_HIP;
        }
    }
    std::vector<ncclComm_t> comms(distinct.size(), nullptr);
    const ncclResult_t cr = ncclCommInitAll(comms.data(), (int)distinct.size(), distinct.data());
    if (cr != ncclSuccess) {
        // (no context to carry the message: the caller gets the status, the RCCL text goes to stderr)
        fprintf(stderr, "[drt_hip] drt_hip_create_group: ncclCommInitAll over %zu devices failed: %s\n", distinct.size(), ncclGetErrorString(cr));
        for (ncclComm_t c : comms)
            if (c)
                (void)ncclCommAbort(c);
        drt_hip_destroy(g);             // (destroys the members created so far; none of them holds a communicator yet)
        return DRT_ERR_COMM;
    }
    for (int i = 0, k = 0; i < n_devices; ++i)
        if (g->leader[i] == i) {
            g->members[i]->comm = comms[k];
            g->members[i]->comm_rank = k;
            g->members[i]->comm_size = (int)distinct.size();
            ++k;
        }
    *out = g;
    return DRT_OK;
}

int drt_hip_group_size(const drt_hip_ctx* ctx) { return ctx ? (ctx->members.empty() ? 1 : (int)ctx->members.size()) : 0; }

int drt_hip_upload_scene(drt_hip_ctx* ctx, const drt_scene_desc* s)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    if (ctx->members.empty())
        return upload_scene_one(ctx, s);
    ctx->has_scene = false;
    for (drt_hip_ctx* m : ctx->members) {
        const int rc = upload_scene_one(m, s);
        if (rc != DRT_OK) {
            ctx->err = m->err;
            return rc;
        }
    }
    ctx->has_scene = true;
    return DRT_OK;
}

int drt_hip_set_specialisation(drt_hip_ctx* ctx, int mode)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    if (mode < DRT_SPECIALISE_GENERIC || mode > DRT_SPECIALISE_NOW)
        return fail(ctx, DRT_ERR_INVALID, "set_specialisation: unknown mode");
    ctx->jit_mode = mode;
    for (drt_hip_ctx* m : ctx->members)
        m->jit_mode = mode;
    return DRT_OK;
}

int drt_hip_update_params(drt_hip_ctx* ctx, const double* params)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    if (ctx->members.empty())
        return update_params_one(ctx, params);
    for (drt_hip_ctx* m : ctx->members) {
        const int rc = update_params_one(m, params);
        if (rc != DRT_OK) {
            ctx->err = m->err;
            return rc;
        }
    }
    return DRT_OK;
}

void* drt_hip_stream(drt_hip_ctx* ctx)
{
    if (!ctx)
        return nullptr;
    return (void*)(ctx->members.empty() ? ctx->stream : ctx->members[0]->stream);
}

int drt_hip_synchronize(drt_hip_ctx* ctx)
{
    if (!ctx)
        return DRT_ERR_INVALID;
    if (!ctx->members.empty()) {
        for (drt_hip_ctx* m : ctx->members) {
            const int rc = drt_hip_synchronize(m);
            if (rc != DRT_OK) {
                ctx->err = m->err;
                return rc;
            }
        }
        return DRT_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->copy_stream)
        HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
    return DRT_OK;
}

#ifdef DRT_BVH_STATS
// debug build only: read and clear the traversal counters of k_intersect_mesh (drt_kernels.h)
extern "C" int drt_hip_debug_bvh_stats(unsigned long long* out16)
{
    (void)hipDeviceSynchronize();
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_bvh_stats), 16 * sizeof(unsigned long long)) != hipSuccess)
        return -1;
    unsigned long long zero[16] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_bvh_stats), zero, sizeof zero);
    return 0;
}
#endif

#ifdef DRT_BVH_STATS
extern "C" int drt_hip_debug_bvh_hist(unsigned long long* out24)
{
    (void)hipDeviceSynchronize();
    if (hipMemcpyFromSymbol(out24, HIP_SYMBOL(g_bvh_hist), 24 * sizeof(unsigned long long)) != hipSuccess)
        return -1;
    unsigned long long zero[24] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_bvh_hist), zero, sizeof zero);
    return 0;
}
#endif
#ifdef DRT_WALK_TIMES
// debug build only: start / counters-dry / exit time of every wave of the last k_intersect_mesh launch (drt_kernels.h)
extern "C" int drt_hip_debug_walk_times(unsigned long long* out, int n_waves)
{
    (void)hipDeviceSynchronize();
    if (n_waves > 8192) n_waves = 8192;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_walk_times), (size_t)n_waves * 3 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif

// hiprtc needs no device: the build container checks that the embedded headers still compile under it (tests/test_abi.py).
// Returns the size of the code object, or a negative status with the compiler's output in `log`.
// (user_header: caller-defined kinds as drt_hip_upload_scene writes them for hiprtc, NULL: none)
extern "C" int drt_hip_debug_jit_compile_with(const char* arch, const char* name_expr, const char* user_header, double* ms, char* log, int log_cap);
extern "C" int drt_hip_debug_jit_compile(const char* arch, const char* name_expr, double* ms, char* log, int log_cap)
{
    return drt_hip_debug_jit_compile_with(arch, name_expr, nullptr, ms, log, log_cap);
}
extern "C" int drt_hip_debug_jit_compile_with(const char* arch, const char* name_expr, const char* user_header, double* ms, char* log, int log_cap)
{
    if (!arch || !name_expr)
        return DRT_ERR_INVALID;
    const drt_jit::EntryPtr e = drt_jit::compile(arch, name_expr, user_header ? user_header : "");
    const drt_jit::Code& c = e->code;
    if (ms)
        *ms = c.ms;
    if (log && log_cap > 0) {
        strncpy(log, c.log.c_str(), (size_t)log_cap - 1);
        log[log_cap - 1] = 0;
    }
    return c.ok ? (int)c.bin.size() : DRT_ERR_UNSUPPORTED;
}

const char* drt_hip_last_error(drt_hip_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

const char* drt_hip_kernel_name(int k)
{
    static const char* names[DRT_K_COUNT] = {"k_raygen", "k_intersect", "k_shade", "k_film",
                                             "k_backward", "k_gradreduce", "k_intersect_mesh", "k_path"};
    return (k >= 0 && k < DRT_K_COUNT) ? names[k] : "";
}

} // extern "C"

