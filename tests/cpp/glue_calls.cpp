// What the host glue (include/drt/hip.hpp) sends through the C ABI and what it does with the answers, without a device: this
// program DEFINES the drt_hip_* functions the header calls -- recording stubs in the place of libdrt_hip.so, which is not linked.
// Every stub keeps the drt_render_params and the drt_camera_desc it was given and which of its pointers were NULL, and writes a
// pattern into every output buffer.  Every entry point of drt::hip is then called with an Options whose fields are all off their
// defaults, and the recorded calls, the caller's arrays, grad() and Stats are compared with literals.
// Prints "ok" and exits 0, or reports the first failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "drt/bxdf.hpp"
#include "drt/camera.hpp"
#include "drt/dual.hpp"
#include "drt/emitter.hpp"
#include "drt/hip.hpp"
#include "drt/pathtracer.hpp"
#include "drt/shape.hpp"
#include "drt/vector.hpp"

using namespace drt;

// ---- the recording stubs ------------------------------------------------------------------------------------------------
struct drt_hip_ctx {
    std::vector<int> devices;
    int n_params = 0;
};

struct Call {
    std::string fn;
    drt_hip_ctx* ctx = nullptr;
    drt_render_params rp{};
    drt_camera_desc cam{};
    int param = -2;
    bool adjoint_null = true, out_rgb_null = true, out_second_null = true, grads_null = true, stats_null = true;
    bool target_null = true, residual_null = true, A_null = true, b_null = true, loss_null = true, jacobian_null = true;
    const void* out_rgb = nullptr;
    std::vector<float> image_in;      // adjoint, target or residual, as the stub saw it
    std::vector<double> tangent_in;
};

static std::vector<Call> g_calls;          // the render calls
static std::vector<std::string> g_log;     // everything else: "create 3", "destroy", "upload", "update", "pin 18432", "unpin", "wait 1 stats"
struct Frame { float* rgb; double* grads; int npix, n_params; };
static std::vector<Frame> g_frames;        // by ticket - 1

static float pat_img(std::size_t i) { return 1.f + 0.5f * float(i); }
static float pat_second(std::size_t i) { return 2.f + 0.25f * float(i); }       // gradient image, float tangent image
static double pat_img_d(std::size_t i) { return 3. + 0.125 * double(i); }       // drt_hip_render_tangent_double's
static double pat_second_d(std::size_t i) { return 4. + 0.0625 * double(i); }
static double pat_grad(std::size_t i) { return 10. + double(i); }
static double pat_A(std::size_t i) { return 100. + double(i); }
static double pat_b(std::size_t i) { return 200. + double(i); }
static double pat_loss(std::size_t i) { return 300. + double(i); }

static void fill_stats(drt_hip_stats* st)
{
    if (!st)
        return;
    std::memset(st, 0, sizeof *st);
    st->paths = 11;
    st->segments = 22;
    st->capped_paths = 33;
    st->ms_total = 44.5;
}

static Call& record(const char* fn, drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp)
{
    g_calls.emplace_back();
    Call& c = g_calls.back();
    c.fn = fn;
    c.ctx = ctx;
    c.rp = *rp;
    c.cam = *cam;
    return c;
}

static std::size_t floats_of(const drt_camera_desc* cam) { return (std::size_t)cam->width * (std::size_t)cam->height * 3; }

extern "C" {

int drt_hip_create(int device_id, drt_hip_ctx** out)
{
    *out = new drt_hip_ctx();
    (*out)->devices = {device_id};
    g_log.push_back("create " + std::to_string(device_id));
    return DRT_OK;
}

int drt_hip_create_group(const int* device_ids, int n_devices, drt_hip_ctx** out)
{
    *out = new drt_hip_ctx();
    std::string s = "create_group";
    for (int i = 0; i < n_devices; ++i) {
        (*out)->devices.push_back(device_ids[i]);
        s += " " + std::to_string(device_ids[i]);
    }
    g_log.push_back(s);
    return DRT_OK;
}

void drt_hip_destroy(drt_hip_ctx* ctx)
{
    g_log.push_back("destroy");
    delete ctx;
}

int drt_hip_upload_scene(drt_hip_ctx* ctx, const drt_scene_desc* scene)
{
    ctx->n_params = scene->n_params;
    g_log.push_back("upload " + std::to_string(scene->n_shapes) + " " + std::to_string(scene->n_params));
    return DRT_OK;
}

int drt_hip_update_params(drt_hip_ctx*, const double*)
{
    g_log.push_back("update");
    return DRT_OK;
}

const char* drt_hip_last_error(drt_hip_ctx*) { return "stub"; }

int drt_hip_pin_host(drt_hip_ctx*, void*, size_t bytes)
{
    g_log.push_back("pin " + std::to_string(bytes));
    return DRT_OK;
}

int drt_hip_unpin_host(drt_hip_ctx*, void*)
{
    g_log.push_back("unpin");
    return DRT_OK;
}

int drt_hip_render(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, const float* adjoint_rgb, float* out_rgb,
                   double* out_param_grad, drt_hip_stats* stats)
{
    Call& c = record("render", ctx, cam, rp);
    c.adjoint_null = !adjoint_rgb; c.out_rgb_null = !out_rgb; c.grads_null = !out_param_grad; c.stats_null = !stats;
    c.out_rgb = out_rgb;
    if (adjoint_rgb)
        c.image_in.assign(adjoint_rgb, adjoint_rgb + floats_of(cam));
    for (std::size_t i = 0; out_rgb && i < floats_of(cam); ++i)
        out_rgb[i] = pat_img(i);
    for (int i = 0; out_param_grad && i < ctx->n_params * 3; ++i)
        out_param_grad[i] = pat_grad((std::size_t)i);
    fill_stats(stats);
    return DRT_OK;
}

int drt_hip_render_async(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, const float* adjoint_rgb, float* out_rgb,
                         double* out_param_grad, uint64_t* ticket)
{
    Call& c = record("render_async", ctx, cam, rp);
    c.adjoint_null = !adjoint_rgb; c.out_rgb_null = !out_rgb; c.grads_null = !out_param_grad;
    c.out_rgb = out_rgb;
    if (adjoint_rgb)
        c.image_in.assign(adjoint_rgb, adjoint_rgb + floats_of(cam));
    g_frames.push_back(Frame{out_rgb, out_param_grad, cam->width * cam->height, ctx->n_params});
    *ticket = g_frames.size();
    return DRT_OK;
}

// (like the library: the frame's results reach the caller's buffers HERE)
int drt_hip_wait(drt_hip_ctx*, uint64_t ticket, drt_hip_stats* stats)
{
    g_log.push_back("wait " + std::to_string(ticket) + (stats ? " stats" : ""));
    const Frame& f = g_frames[ticket - 1];
    for (std::size_t i = 0; f.rgb && i < (std::size_t)f.npix * 3; ++i)
        f.rgb[i] = pat_img(i);
    for (int i = 0; f.grads && i < f.n_params * 3; ++i)
        f.grads[i] = pat_grad((std::size_t)i);
    fill_stats(stats);
    return DRT_OK;
}

int drt_hip_render_gradient_image(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t param,
                                  const float* adjoint_rgb, float* out_rgb, float* out_grad_rgb, drt_hip_stats* stats)
{
    Call& c = record("render_gradient_image", ctx, cam, rp);
    c.param = param;
    c.adjoint_null = !adjoint_rgb; c.out_rgb_null = !out_rgb; c.out_second_null = !out_grad_rgb; c.stats_null = !stats;
    for (std::size_t i = 0; i < floats_of(cam); ++i) {
        if (out_rgb) out_rgb[i] = pat_img(i);
        if (out_grad_rgb) out_grad_rgb[i] = pat_second(i);
    }
    fill_stats(stats);
    return DRT_OK;
}

int drt_hip_render_tangent(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, const double* param_tangent,
                           float* out_rgb, float* out_tangent_rgb, drt_hip_stats* stats)
{
    Call& c = record("render_tangent", ctx, cam, rp);
    c.out_rgb_null = !out_rgb; c.out_second_null = !out_tangent_rgb; c.stats_null = !stats;
    if (param_tangent)
        c.tangent_in.assign(param_tangent, param_tangent + ctx->n_params * 3);
    for (std::size_t i = 0; i < floats_of(cam); ++i) {
        if (out_rgb) out_rgb[i] = pat_img(i);
        if (out_tangent_rgb) out_tangent_rgb[i] = pat_second(i);
    }
    fill_stats(stats);
    return DRT_OK;
}

int drt_hip_render_tangent_double(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, const double* param_tangent,
                                  double* out_rgb, double* out_tangent_rgb, drt_hip_stats* stats)
{
    Call& c = record("render_tangent_double", ctx, cam, rp);
    c.out_rgb_null = !out_rgb; c.out_second_null = !out_tangent_rgb; c.stats_null = !stats;
    if (param_tangent)
        c.tangent_in.assign(param_tangent, param_tangent + ctx->n_params * 3);
    for (std::size_t i = 0; i < floats_of(cam); ++i) {
        if (out_rgb) out_rgb[i] = pat_img_d(i);
        if (out_tangent_rgb) out_tangent_rgb[i] = pat_second_d(i);
    }
    fill_stats(stats);
    return DRT_OK;
}

int drt_hip_render_normal_equations(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, const float* target_rgb,
                                    const float* residual_rgb, float* out_rgb, double* out_A, double* out_b, double* out_loss,
                                    float* out_jacobian, drt_hip_stats* stats)
{
    Call& c = record("render_normal_equations", ctx, cam, rp);
    c.target_null = !target_rgb; c.residual_null = !residual_rgb; c.out_rgb_null = !out_rgb; c.A_null = !out_A; c.b_null = !out_b;
    c.loss_null = !out_loss; c.jacobian_null = !out_jacobian; c.stats_null = !stats;
    const float* in = target_rgb ? target_rgb : residual_rgb;
    if (in)
        c.image_in.assign(in, in + floats_of(cam));
    const std::size_t P = (std::size_t)ctx->n_params;
    for (std::size_t i = 0; out_rgb && i < floats_of(cam); ++i)
        out_rgb[i] = pat_img(i);
    for (std::size_t i = 0; out_A && i < 3 * P * P; ++i)
        out_A[i] = pat_A(i);
    for (std::size_t i = 0; out_b && i < 3 * P; ++i)
        out_b[i] = pat_b(i);
    for (std::size_t i = 0; out_loss && i < 3; ++i)
        out_loss[i] = pat_loss(i);
    fill_stats(stats);
    return DRT_OK;
}

} // extern "C"

// ---- the checks ----------------------------------------------------------------------------------------------------------
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

template <typename F>
static bool throws_exactly(F&& f, const char* message)
{
    try {
        f();
    } catch (const std::runtime_error& e) {
        if (std::strcmp(e.what(), message) == 0)
            return true;
        std::printf("threw \"%s\", not \"%s\"\n", e.what(), message);
        return false;
    }
    std::printf("did not throw (expected \"%s\")\n", message);
    return false;
}

// (every entry point sends n_shards = 1 and the caller's band_rows: whole frames -- the library normalises n_shards <= 1 to 1 and reads
//  band_rows only where bands are dealt out, which is a group context's business)
static bool rp_is(const drt_render_params& r, int spp, int min_bounces, double absorb, int max_depth, unsigned seed, int shard, int n_shards,
                  int band_rows, unsigned flags, long long batch_paths, int bounces_per_launch)
{
    const bool ok = r.spp == spp && r.min_bounces == min_bounces && r.absorb == absorb && r.max_depth == max_depth && r.seed == seed &&
                    r.shard == shard && r.n_shards == n_shards && r.band_rows == band_rows && r.flags == flags &&
                    r.batch_paths == batch_paths && r.bounces_per_launch == bounces_per_launch && r.reserved == 0;
    if (!ok)
        std::printf("drt_render_params: spp %d min_bounces %d absorb %g max_depth %d seed %u shard %d n_shards %d band_rows %d flags 0x%x "
                    "batch_paths %lld bounces_per_launch %d reserved %d\n", r.spp, r.min_bounces, r.absorb, r.max_depth, r.seed, r.shard,
                    r.n_shards, r.band_rows, r.flags, (long long)r.batch_paths, r.bounces_per_launch, r.reserved);
    return ok;
}

static bool same_camera(const drt_camera_desc& a, const drt_camera_desc& b)
{
    bool ok = a.width == b.width && a.height == b.height && a.vfov == b.vfov;
    for (int i = 0; i < 3; ++i)
        ok = ok && a.eye[i] == b.eye[i] && a.forward[i] == b.forward[i] && a.right[i] == b.right[i] && a.up[i] == b.up[i];
    return ok;
}

static bool stats_are(const hip::Stats& st, unsigned long long capped)
{
    const bool ok = st.paths == 11 && st.segments == 22 && st.capped_paths == capped && st.ms == 44.5;
    if (!ok)
        std::printf("Stats: paths %llu segments %llu capped_paths %llu ms %g\n", st.paths, st.segments, st.capped_paths, st.ms);
    return ok;
}

static bool log_is(std::initializer_list<const char*> want)
{
    bool ok = g_log.size() == want.size();
    std::size_t i = 0;
    for (const char* w : want) {
        if (ok && g_log[i] != w)
            ok = false;
        ++i;
    }
    if (!ok) {
        std::printf("log:");
        for (const std::string& s : g_log)
            std::printf(" [%s]", s.c_str());
        std::printf("\n");
    }
    g_log.clear();
    return ok;
}

static const int W = 48, H = 32, NPIX = W * H;

// the three-shape scene of test_a_dropped_frame_does_not_block_the_pooled_context; the emission takes no gradient
template <typename T>
struct World {
    Vector<T, 3, true> white{Vector<T, 3>{T(0.5), T(0.5), T(0.5)}, true}, emission{Vector<T, 3>(T(1)), false};
    std::shared_ptr<BxDF<T>> mat = std::make_shared<DiffuseBxDF<T>>(white);
    std::shared_ptr<Emitter<T>> em = std::make_shared<AreaEmitter<T>>(emission);
    Sphere<T> ball{Vector<T, 3>{0., 0., 3.}, 1., mat};
    Plane<T> floor_{Vector<T, 3>{0., 1., 0.}, -3., mat};
    Sphere<T> light{Vector<T, 3>{0., 3., 3.}, 1., nullptr, em};
    Scene<T> scene{&ball, &floor_, &light};
    Camera<T> cam{(std::size_t)W, (std::size_t)H};
    Pathtracer<T> tracer{0.75, 3};
    World() { cam.look_at(Vector<T, 3>{0, 0, 0}, Vector<T, 3>{0, 0, 1}); }
};

// every field off its default
static hip::Options options(bool f64, bool reuse)
{
    hip::Options opt;
    opt.seed = 7;
    opt.max_depth = 9;
    opt.devices = {3};
    opt.band_rows = 5;
    opt.f64 = f64;
    opt.batch_paths = 4096;
    opt.bounces_per_launch = 2;
    opt.reuse_context = reuse;
    return opt;
}

using V3 = Vector<double, 3>;

static bool image_is(const std::vector<V3>& img, float (*pat)(std::size_t))
{
    for (std::size_t i = 0; i < img.size(); ++i)
        for (int c = 0; c < 3; ++c)
            if (img[i][c] != double(pat(i * 3 + c)))
                return false;
    return true;
}

static bool image_is_d(const std::vector<V3>& img, double (*pat)(std::size_t))
{
    for (std::size_t i = 0; i < img.size(); ++i)
        for (int c = 0; c < 3; ++c)
            if (img[i][c] != pat(i * 3 + c))
                return false;
    return true;
}

static bool untouched(const std::vector<V3>& img)
{
    for (const V3& p : img)
        for (int c = 0; c < 3; ++c)
            if (p[c] != -1.)
                return false;
    return true;
}

static bool floats_of_image(const std::vector<float>& got, const std::vector<V3>& img)
{
    if (got.size() != img.size() * 3)
        return false;
    for (std::size_t i = 0; i < img.size(); ++i)
        for (int c = 0; c < 3; ++c)
            if (got[i * 3 + c] != float(img[i][c]))
                return false;
    return true;
}

static std::vector<V3> some_image(double scale)
{
    std::vector<V3> a((std::size_t)NPIX);
    for (std::size_t i = 0; i < a.size(); ++i)
        a[i] = V3{scale * double(i) + 0.1, scale * double(i) + 0.2, 0.3 - scale * double(i)};   // (not exact in float)
    return a;
}

struct Mode { bool backward, unbiased, sample_loss_l2; unsigned flags; };
static const Mode MODES[6] = {{false, false, false, 0x0u}, {true, false, false, 0x1u}, {false, true, false, 0x0u},
                              {false, false, true, 0x0u}, {true, true, false, 0x21u}, {true, false, true, 0x401u}};

static int render_checks()
{
    using T = double;
    World<T> w;
    const drt_camera_desc cd = hip::describe(w.cam);
    const std::vector<V3> adjoint = some_image(1e-3);
    double grown = 0;       // how often the pattern has been added to white.grad()
    for (int f64 = 0; f64 < 2; ++f64)
        for (const Mode& m : MODES)
            for (int with_adjoint = 0; with_adjoint < 2; ++with_adjoint) {
                hip::Options opt = options(f64 != 0, false);
                opt.backward = m.backward; opt.unbiased = m.unbiased; opt.sample_loss_l2 = m.sample_loss_l2;
                std::vector<V3> img((std::size_t)NPIX, V3(-1.));
                g_calls.clear();
                const hip::Stats st = hip::render(w.scene, w.cam, w.tracer, 6, img.data(), opt, with_adjoint ? adjoint.data() : nullptr);
                CHECK(log_is({"create 3", "upload 3 2", "destroy"}));          // a context of its own: no pinned frame
                CHECK(g_calls.size() == 1 && g_calls[0].fn == "render");
                const Call& c = g_calls[0];
                CHECK(rp_is(c.rp, 6, 3, 0.75, 9, 7u, 0, 1, 5, m.flags | (f64 ? 0x10u : 0u), 4096, 2));
                CHECK(same_camera(c.cam, cd));
                CHECK(c.adjoint_null == !with_adjoint && !c.out_rgb_null && c.grads_null == !m.backward && !c.stats_null);
                CHECK(!with_adjoint || floats_of_image(c.image_in, adjoint));
                CHECK(image_is(img, pat_img));
                CHECK(stats_are(st, 33));
                grown += m.backward ? 1 : 0;
                for (int ch = 0; ch < 3; ++ch)
                    CHECK(w.white.grad()[ch] == grown * pat_grad((std::size_t)ch));      // accumulated; parameter 0
                CHECK(throws_exactly([&] { (void)w.emission.grad(); }, "Vector has no gradient (not a variable)"));   // skipped: parameter 1
            }
    CHECK(grown == 12);

    // the pooled context: made once, the scene uploaded once, the frame buffer the context's own and pinned
    {
        hip::Options opt = options(false, true);
        opt.backward = true;
        std::vector<V3> img((std::size_t)NPIX, V3(-1.));
        g_calls.clear();
        hip::render(w.scene, w.cam, w.tracer, 6, img.data(), opt);
        CHECK(log_is({"create 3", "upload 3 2", "pin 18432"}));
        hip::render(w.scene, w.cam, w.tracer, 6, img.data(), opt);
        CHECK(log_is({}));
        w.white[1] = 0.25;
        hip::render(w.scene, w.cam, w.tracer, 6, img.data(), opt);
        CHECK(log_is({"update"}));
        CHECK(g_calls.size() == 3 && g_calls[0].out_rgb == g_calls[1].out_rgb && g_calls[1].out_rgb == g_calls[2].out_rgb);
        CHECK(g_calls[0].ctx == g_calls[2].ctx && g_calls[2].out_rgb != (const void*)img.data());
        CHECK(rp_is(g_calls[2].rp, 6, 3, 0.75, 9, 7u, 0, 1, 5, 0x1u, 4096, 2));
        CHECK(image_is(img, pat_img));
        grown += 3;
        for (int ch = 0; ch < 3; ++ch)
            CHECK(w.white.grad()[ch] == grown * pat_grad((std::size_t)ch));
        // several devices: one group context, its frame buffer not pinned
        opt.devices = {3, 4};
        hip::render(w.scene, w.cam, w.tracer, 6, img.data(), opt);
        CHECK(log_is({"create_group 3 4", "upload 3 2"}));
        CHECK(g_calls.size() == 4 && rp_is(g_calls[3].rp, 6, 3, 0.75, 9, 7u, 0, 1, 5, 0x1u, 4096, 2));
        grown += 1;
        hip::release_contexts();
        CHECK(log_is({"destroy", "destroy"}));
        opt.devices.clear();
        CHECK(throws_exactly([&] { hip::render(w.scene, w.cam, w.tracer, 6, img.data(), opt); }, "drt::hip::render: no device given"));
        CHECK(log_is({}));
    }
    return 0;
}

static int submit_checks()
{
    using T = double;
    World<T> w;
    const drt_camera_desc cd = hip::describe(w.cam);
    const std::vector<V3> adjoint = some_image(1e-3);
    double grown = 0;
    bool first = true;
    for (int f64 = 0; f64 < 2; ++f64)
        for (const Mode& m : MODES)
            for (int with_adjoint = 0; with_adjoint < 2; ++with_adjoint) {
                hip::Options opt = options(f64 != 0, false);          // (frames in flight are the pooled context's whatever reuse_context says)
                opt.backward = m.backward; opt.unbiased = m.unbiased; opt.sample_loss_l2 = m.sample_loss_l2;
                std::vector<V3> img((std::size_t)NPIX, V3(-1.));
                g_calls.clear();
                hip::Pending<T> p = hip::submit(w.scene, w.cam, w.tracer, 6, img.data(), opt, with_adjoint ? adjoint.data() : nullptr);
                CHECK(first ? log_is({"create 3", "upload 3 2"}) : log_is({}));
                first = false;
                CHECK(p.valid() && g_calls.size() == 1 && g_calls[0].fn == "render_async");
                const Call& c = g_calls[0];
                CHECK(rp_is(c.rp, 6, 3, 0.75, 9, 7u, 0, 1, 5, m.flags | (f64 ? 0x10u : 0u), 4096, 2));
                CHECK(same_camera(c.cam, cd));
                CHECK(c.adjoint_null == !with_adjoint && !c.out_rgb_null && c.grads_null == !m.backward);
                CHECK(!with_adjoint || floats_of_image(c.image_in, adjoint));
                CHECK(untouched(img));
                for (int ch = 0; ch < 3; ++ch)
                    CHECK(w.white.grad()[ch] == grown * pat_grad((std::size_t)ch));      // nothing before get()
                const hip::Stats st = p.get();
                CHECK(!p.valid());
                CHECK(log_is({("wait " + std::to_string(g_frames.size()) + " stats").c_str()}));
                CHECK(image_is(img, pat_img));
                CHECK(stats_are(st, 33));
                grown += m.backward ? 1 : 0;
                for (int ch = 0; ch < 3; ++ch)
                    CHECK(w.white.grad()[ch] == grown * pat_grad((std::size_t)ch));
                CHECK(throws_exactly([&] { (void)w.emission.grad(); }, "Vector has no gradient (not a variable)"));
                CHECK(throws_exactly([&] { p.get(); }, "drt::hip::Pending::get: no frame"));
            }
    CHECK(grown == 12 && g_frames.size() == 24);
    {
        hip::Options opt = options(false, true);
        opt.backward = true;
        std::vector<V3> img((std::size_t)NPIX, V3(-1.));
        {
            hip::Pending<T> p[4];
            for (int i = 0; i < 4; ++i)
                p[i] = hip::submit(w.scene, w.cam, w.tracer, 6, img.data(), opt);
            CHECK(throws_exactly([&] { hip::submit(w.scene, w.cam, w.tracer, 6, img.data(), opt); },
                                 "drt::hip::submit: four frames are in flight on this device -- get() the oldest one first"));
            CHECK(log_is({}));
            p[0].get();
            CHECK(log_is({"wait 25 stats"}));
            grown += 1;
        }       // the other three are dropped: waited for, nothing accumulated (destroyed last to first)
        CHECK(log_is({"wait 28", "wait 27", "wait 26"}));
        for (int ch = 0; ch < 3; ++ch)
            CHECK(w.white.grad()[ch] == grown * pat_grad((std::size_t)ch));
        opt.devices = {3, 4};
        CHECK(throws_exactly([&] { hip::submit(w.scene, w.cam, w.tracer, 6, img.data(), opt); },
                             "drt::hip::submit: one device (frames in flight are per device context)"));
        opt.devices.clear();
        CHECK(throws_exactly([&] { hip::submit(w.scene, w.cam, w.tracer, 6, img.data(), opt); },
                             "drt::hip::submit: one device (frames in flight are per device context)"));
        hip::release_contexts();
        CHECK(log_is({"destroy"}));
    }
    return 0;
}

static int gradient_image_checks()
{
    using T = double;
    World<T> w;
    const drt_camera_desc cd = hip::describe(w.cam);
    for (int f64 = 0; f64 < 2; ++f64)
        for (int reuse = 0; reuse < 2; ++reuse)
            for (int with_img = 0; with_img < 2; ++with_img) {
                const hip::Options opt = options(f64 != 0, reuse != 0);
                std::vector<V3> img((std::size_t)NPIX, V3(-1.)), gimg((std::size_t)NPIX, V3(-1.));
                g_calls.clear();
                const Vector<T, 3, true>& param = with_img ? w.emission : w.white;
                const hip::Stats st = hip::render_gradient_image(w.scene, w.cam, w.tracer, 6, param, with_img ? img.data() : nullptr, gimg.data(), opt);
                if (!reuse)
                    CHECK(log_is({"create 3", "upload 3 2", "destroy"}));
                else
                    CHECK(f64 == 0 && with_img == 0 ? log_is({"create 3", "upload 3 2"}) : log_is({}));
                CHECK(g_calls.size() == 1 && g_calls[0].fn == "render_gradient_image");
                const Call& c = g_calls[0];
                // (bounces_per_launch is NOT forwarded: the gradient image keeps the automatic route)
                CHECK(rp_is(c.rp, 6, 3, 0.75, 9, 7u, 0, 1, 5, f64 ? 0x10u : 0u, 4096, 0));
                CHECK(same_camera(c.cam, cd));
                CHECK(c.param == (with_img ? 1 : 0));
                CHECK(c.adjoint_null && !c.out_rgb_null && !c.out_second_null && !c.stats_null);
                CHECK(with_img ? image_is(img, pat_img) : untouched(img));
                CHECK(image_is(gimg, pat_second));
                CHECK(stats_are(st, 33));
                CHECK(w.white.grad()[0] == 0. && w.white.grad()[1] == 0. && w.white.grad()[2] == 0.);
            }
    hip::release_contexts();
    CHECK(log_is({"destroy"}));
    {
        std::vector<V3> gimg((std::size_t)NPIX);
        Vector<T, 3, true> stranger(Vector<T, 3>(0.25), true);
        hip::Options opt = options(false, false);
        CHECK(throws_exactly([&] { hip::render_gradient_image(w.scene, w.cam, w.tracer, 6, stranger, (V3*)nullptr, gimg.data(), opt); },
                             "drt::hip::render_gradient_image: the parameter is not used by the scene"));
        CHECK(log_is({}));
        opt.devices.clear();           // this entry point falls back to device 0; of several it takes the first
        hip::render_gradient_image(w.scene, w.cam, w.tracer, 6, w.white, (V3*)nullptr, gimg.data(), opt);
        CHECK(log_is({"create 0", "upload 3 2", "destroy"}));
        opt.devices = {5, 6};
        hip::render_gradient_image(w.scene, w.cam, w.tracer, 6, w.white, (V3*)nullptr, gimg.data(), opt);
        CHECK(log_is({"create 5", "upload 3 2", "destroy"}));
    }
    return 0;
}

static int tangent_checks()
{
    using T = double;
    World<T> w;
    const drt_camera_desc cd = hip::describe(w.cam);
    // white listed twice (adds up), the emission once
    const std::vector<std::pair<Vector<T, 3, true>, V3>> tangents = {{w.white, V3{0.5, -1., 2.}}, {w.emission, V3{0., 1.5, 0.25}}, {w.white, V3{0.25, 0.25, -4.}}};
    const double v_want[6] = {0.75, -0.75, -2., 0., 1.5, 0.25};
    for (int f64 = 0; f64 < 2; ++f64)
        for (int reuse = 0; reuse < 2; ++reuse)
            for (int with_img = 0; with_img < 2; ++with_img) {
                const hip::Options opt = options(f64 != 0, reuse != 0);
                std::vector<V3> img((std::size_t)NPIX, V3(-1.)), timg((std::size_t)NPIX, V3(-1.));
                g_calls.clear();
                const hip::Stats st = hip::render_tangent(w.scene, w.cam, w.tracer, 6, tangents, with_img ? img.data() : nullptr, timg.data(), opt);
                if (!reuse)
                    CHECK(log_is({"create 3", "upload 3 2", "destroy"}));
                else
                    CHECK(f64 == 0 && with_img == 0 ? log_is({"create 3", "upload 3 2"}) : log_is({}));
                CHECK(g_calls.size() == 1 && g_calls[0].fn == (f64 ? "render_tangent_double" : "render_tangent"));
                const Call& c = g_calls[0];
                CHECK(rp_is(c.rp, 6, 3, 0.75, 9, 7u, 0, 1, 5, f64 ? 0x10u : 0u, 4096, 2));
                CHECK(same_camera(c.cam, cd));
                CHECK(!c.out_rgb_null && !c.out_second_null && !c.stats_null);
                CHECK(c.tangent_in.size() == 6);
                for (int i = 0; i < 6; ++i)
                    CHECK(c.tangent_in[(std::size_t)i] == v_want[i]);
                if (f64) {
                    CHECK(with_img ? image_is_d(img, pat_img_d) : untouched(img));
                    CHECK(image_is_d(timg, pat_second_d));
                } else {
                    CHECK(with_img ? image_is(img, pat_img) : untouched(img));
                    CHECK(image_is(timg, pat_second));
                }
                CHECK(stats_are(st, 33));
            }
    hip::release_contexts();
    CHECK(log_is({"destroy"}));
    {
        std::vector<V3> img((std::size_t)NPIX), timg((std::size_t)NPIX);
        Vector<T, 3, true> stranger(Vector<T, 3>(0.25), true);
        hip::Options opt = options(false, false);
        CHECK(throws_exactly([&] { hip::render_tangent(w.scene, w.cam, w.tracer, 6, {{stranger, V3(1.)}}, img.data(), timg.data(), opt); },
                             "drt::hip::render_tangent: a listed parameter is not used by the scene"));
        for (int k = 0; k < 3; ++k) {
            hip::Options bad = options(false, false);
            (k == 0 ? bad.backward : k == 1 ? bad.unbiased : bad.sample_loss_l2) = true;
            CHECK(throws_exactly([&] { hip::render_tangent(w.scene, w.cam, w.tracer, 6, tangents, img.data(), timg.data(), bad); },
                                 "drt::hip::render_tangent: forward mode takes no reverse-mode option (backward, unbiased, sample_loss_l2)"));
        }
        CHECK(log_is({}));
        opt.devices.clear();
        hip::render_tangent(w.scene, w.cam, w.tracer, 6, tangents, img.data(), timg.data(), opt);
        CHECK(log_is({"create 0", "upload 3 2", "destroy"}));
    }

    // the same through Dual numbers: the dual parts of the parameters are the direction, the image comes back as Dual(img, tangent)
    using D = Dual<double>;
    using DV = Vector<D, 3>;
    World<D> dw;
    for (int c = 0; c < 3; ++c) {
        dw.white[c] = D(0.5, v_want[c]);
        dw.emission[c] = D(1., v_want[3 + c]);
    }
    for (int f64 = 0; f64 < 2; ++f64) {
        const hip::Options opt = options(f64 != 0, false);
        std::vector<DV> img((std::size_t)NPIX, DV(D(-1.)));
        g_calls.clear();
        const hip::Stats st = hip::render(dw.scene, dw.cam, dw.tracer, 6, img.data(), opt);
        CHECK(log_is({"create 3", "upload 3 2", "destroy"}));
        CHECK(g_calls.size() == 1 && g_calls[0].fn == (f64 ? "render_tangent_double" : "render_tangent"));
        const Call& c = g_calls[0];
        CHECK(rp_is(c.rp, 6, 3, 0.75, 9, 7u, 0, 1, 5, f64 ? 0x10u : 0u, 4096, 2));
        CHECK(same_camera(c.cam, cd));
        CHECK(!c.out_rgb_null && !c.out_second_null && !c.stats_null);
        CHECK(c.tangent_in.size() == 6);
        for (int i = 0; i < 6; ++i)
            CHECK(c.tangent_in[(std::size_t)i] == v_want[i]);
        for (std::size_t i = 0; i < (std::size_t)NPIX; ++i)
            for (int ch = 0; ch < 3; ++ch) {
                CHECK(img[i][ch].real() == (f64 ? pat_img_d(i * 3 + ch) : double(pat_img(i * 3 + ch))));
                CHECK(img[i][ch].dual() == (f64 ? pat_second_d(i * 3 + ch) : double(pat_second(i * 3 + ch))));
            }
        CHECK(stats_are(st, 33));
    }
    {
        std::vector<DV> img((std::size_t)NPIX);
        CHECK(throws_exactly([&] { hip::render(dw.scene, dw.cam, dw.tracer, 6, img.data(), options(false, false), img.data()); },
                             "drt::hip::render: Dual numbers are forward mode: no adjoint image (a reverse-mode notion)"));
        for (int k = 0; k < 3; ++k) {
            hip::Options bad = options(false, false);
            (k == 0 ? bad.backward : k == 1 ? bad.unbiased : bad.sample_loss_l2) = true;
            CHECK(throws_exactly([&] { hip::render(dw.scene, dw.cam, dw.tracer, 6, img.data(), bad); },
                                 "drt::hip::render (Dual): forward mode takes no reverse-mode option (backward, unbiased, sample_loss_l2)"));
        }
        CHECK(log_is({}));
    }
    return 0;
}

static int normal_equations_checks()
{
    using T = double;
    World<T> w;
    const drt_camera_desc cd = hip::describe(w.cam);
    const std::vector<V3> in = some_image(2e-3);
    for (int f64 = 0; f64 < 2; ++f64)
        for (int reuse = 0; reuse < 2; ++reuse)
            for (int residual = 0; residual < 2; ++residual) {
                const hip::Options opt = options(f64 != 0, reuse != 0);
                const bool with_img = residual != 0;
                std::vector<V3> img((std::size_t)NPIX, V3(-1.));
                g_calls.clear();
                const hip::NormalEquations<T> ne = hip::normal_equations(
                    w.scene, w.cam, w.tracer, 6, opt,
                    residual ? hip::TargetOrResidual<T>::residual(in.data()) : hip::TargetOrResidual<T>::target(in.data()), with_img ? img.data() : nullptr);
                if (!reuse)
                    CHECK(log_is({"create 3", "upload 3 2", "destroy"}));
                else
                    CHECK(f64 == 0 && residual == 0 ? log_is({"create 3", "upload 3 2"}) : log_is({}));
                CHECK(g_calls.size() == 1 && g_calls[0].fn == "render_normal_equations");
                const Call& c = g_calls[0];
                CHECK(rp_is(c.rp, 6, 3, 0.75, 9, 7u, 0, 1, 5, f64 ? 0x10u : 0u, 4096, 2));
                CHECK(same_camera(c.cam, cd));
                CHECK(c.target_null == (residual != 0) && c.residual_null == (residual == 0));       // exactly one of the two
                CHECK(!c.out_rgb_null && !c.A_null && !c.b_null && !c.loss_null && c.jacobian_null && !c.stats_null);
                CHECK(floats_of_image(c.image_in, in));
                CHECK(with_img ? image_is(img, pat_img) : untouched(img));
                CHECK(ne.n_params == 2 && ne.A.size() == 12 && ne.b.size() == 6 && ne.loss.size() == 3);
                for (std::size_t i = 0; i < 12; ++i)
                    CHECK(ne.A[i] == pat_A(i));
                for (std::size_t i = 0; i < 6; ++i)
                    CHECK(ne.b[i] == pat_b(i));
                for (std::size_t i = 0; i < 3; ++i)
                    CHECK(ne.loss[i] == pat_loss(i));
                CHECK(ne.requires_grad.size() == 2 && ne.requires_grad[0] == 1 && ne.requires_grad[1] == 0);
                CHECK(ne.handles.size() == 2 && ne.handles[0].id() == w.white.id() && ne.handles[1].id() == w.emission.id());
                CHECK(stats_are(ne.stats, 33));
            }
    hip::release_contexts();
    CHECK(log_is({"destroy"}));
    {
        const auto target = hip::TargetOrResidual<T>::target(in.data());
        for (int k = 0; k < 3; ++k) {
            hip::Options bad = options(false, false);
            (k == 0 ? bad.backward : k == 1 ? bad.unbiased : bad.sample_loss_l2) = true;
            CHECK(throws_exactly([&] { hip::normal_equations(w.scene, w.cam, w.tracer, 6, bad, target); },
                                 "drt::hip::normal_equations: the normal equations take no reverse-mode option (backward, unbiased, sample_loss_l2)"));
        }
        hip::Options opt = options(false, false);
        opt.devices = {3, 4};
        CHECK(throws_exactly([&] { hip::normal_equations(w.scene, w.cam, w.tracer, 6, opt, target); },
                             "drt::hip::normal_equations: the normal equations come from one device (render shards on plain contexts and add them)"));
        opt.devices = {3};
        CHECK(throws_exactly([&] { hip::normal_equations(w.scene, w.cam, w.tracer, 6, opt, hip::TargetOrResidual<T>()); },
                             "drt::hip::normal_equations: the normal equations need a target or a residual image"));
        CHECK(log_is({}));
        opt.devices.clear();
        hip::normal_equations(w.scene, w.cam, w.tracer, 6, opt, target);
        CHECK(log_is({"create 0", "upload 3 2", "destroy"}));
    }
    return 0;
}

int main()
{
    if (render_checks() || submit_checks())
        return 1;
    if (gradient_image_checks() || tangent_checks() || normal_equations_checks())
        return 1;
    std::printf("ok\n");
    return 0;
}
