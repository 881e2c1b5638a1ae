// drt::hip::render_param_sets_along (include/drt/hip.hpp) against recording stubs of the drt_hip_* functions it reaches, in the style of
// param_sets_glue.cpp: libdrt_hip.so is not linked.  The stub keeps the drt_render_params, the camera, the sets, the directions, the
// target and which pointers were NULL, and writes patterns into the outputs; the caller's arrays, sums, Stats and the exceptions' texts
// are compared with literals: the glue adds nothing to the ABI's results.  Prints "ok" and exits 0, or reports the first failure.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "drt/bxdf.hpp"
#include "drt/camera.hpp"
#include "drt/emitter.hpp"
#include "drt/hip.hpp"
#include "drt/pathtracer.hpp"
#include "drt/shape.hpp"
#include "drt/vector.hpp"

using namespace drt;

struct drt_hip_ctx {
    std::vector<int> devices;
    int n_params = 0;
};

struct Call {
    drt_hip_ctx* ctx = nullptr;
    drt_render_params rp{};
    drt_camera_desc cam{};
    int n_sets = -1;
    bool sets_null = true, dirs_null = true, target_null = true, images_null = true, tangents_null = true, loss_null = true, dloss_null = true,
         curv_null = true, stats_null = true;
    std::vector<double> sets, dirs;
    std::vector<float> target;
};
static std::vector<Call> g_calls;
static std::vector<std::string> g_log;

static float pat_img(std::size_t i) { return 1.f + 0.5f * float(i); }
static float pat_tan(std::size_t i) { return -2.f - 0.25f * float(i); }
static double pat_loss(std::size_t i) { return 300. + double(i); }
static double pat_dloss(std::size_t i) { return -40. - double(i); }
static double pat_curv(std::size_t i) { return 7. + 0.5 * double(i); }
static std::size_t floats_of(const drt_camera_desc* cam) { return (std::size_t)cam->width * (std::size_t)cam->height * 3; }

extern "C" {

int drt_hip_create(int device_id, drt_hip_ctx** out)
{
    *out = new drt_hip_ctx();
    (*out)->devices = {device_id};
    g_log.push_back("create " + std::to_string(device_id));
    return DRT_OK;
}
int drt_hip_create_group(const int*, int, drt_hip_ctx** out)
{
    *out = new drt_hip_ctx();
    g_log.push_back("create_group");
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
int drt_hip_pin_host(drt_hip_ctx*, void*, size_t) { return DRT_OK; }
int drt_hip_unpin_host(drt_hip_ctx*, void*) { return DRT_OK; }

static int g_answer = DRT_OK;
int drt_hip_render_param_sets_along(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_sets,
                                    const double* param_sets, const double* param_tangents, const float* target_rgb, float* out_images,
                                    float* out_tangents, double* out_loss, double* out_dloss, double* out_curv, drt_hip_stats* stats)
{
    g_calls.emplace_back();
    Call& c = g_calls.back();
    c.ctx = ctx; c.rp = *rp; c.cam = *cam; c.n_sets = n_sets;
    c.sets_null = !param_sets; c.dirs_null = !param_tangents; c.target_null = !target_rgb; c.images_null = !out_images;
    c.tangents_null = !out_tangents; c.loss_null = !out_loss; c.dloss_null = !out_dloss; c.curv_null = !out_curv; c.stats_null = !stats;
    const std::size_t n = (std::size_t)n_sets * (std::size_t)ctx->n_params * 3;
    if (param_sets)
        c.sets.assign(param_sets, param_sets + n);
    if (param_tangents)
        c.dirs.assign(param_tangents, param_tangents + n);
    if (target_rgb)
        c.target.assign(target_rgb, target_rgb + floats_of(cam));
    for (std::size_t i = 0; out_images && i < (std::size_t)n_sets * floats_of(cam); ++i)
        out_images[i] = pat_img(i);
    for (std::size_t i = 0; out_tangents && i < (std::size_t)n_sets * floats_of(cam); ++i)
        out_tangents[i] = pat_tan(i);
    for (std::size_t i = 0; i < (std::size_t)n_sets * 3; ++i) {
        if (out_loss) out_loss[i] = pat_loss(i);
        if (out_dloss) out_dloss[i] = pat_dloss(i);
        if (out_curv) out_curv[i] = pat_curv(i);
    }
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->paths = 11; stats->segments = 22; stats->capped_paths = 33; stats->ms_total = 44.5;
    }
    return g_answer;
}

} // extern "C"

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

static const int W = 12, H = 8, NPIX = W * H;
using V3 = Vector<double, 3>;

// the three-shape scene of glue_calls.cpp: parameters (white, emission)
struct World {
    Vector<double, 3, true> white{V3{0.5, 0.5, 0.5}, true}, emission{V3(1.), false};
    std::shared_ptr<BxDF<double>> mat = std::make_shared<DiffuseBxDF<double>>(white);
    std::shared_ptr<Emitter<double>> em = std::make_shared<AreaEmitter<double>>(emission);
    Sphere<double> ball{V3{0., 0., 3.}, 1., mat};
    Plane<double> floor_{V3{0., 1., 0.}, -3., mat};
    Sphere<double> light{V3{0., 3., 3.}, 1., nullptr, em};
    Scene<double> scene{&ball, &floor_, &light};
    Camera<double> cam{(std::size_t)W, (std::size_t)H};
    Pathtracer<double> tracer{0.75, 3};
    World() { cam.look_at(V3{0, 0, 0}, V3{0, 0, 1}); }
};

static hip::Options options(bool f64, bool reuse)
{
    hip::Options opt;            // every field off its default
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

static int checks()
{
    World w;
    const drt_camera_desc cd = hip::describe(w.cam);
    // set 0: white replaced (listed twice: the last value and direction stand), the emission as in the scene with direction 0;
    // set 1: the emission alone; set 2: empty -- the scene's values, direction 0
    const std::vector<hip::ParamSetAlong<double>> sets = {
        {{w.white, V3{0.1, 0.2, 0.3}, V3{9., 9., 9.}}, {w.white, V3{0.25, 0., 0.75}, V3{1., -2., 0.5}}},
        {{w.emission, V3{2., 3., 4.}, V3{-0.5, 0.25, 8.}}},
        {}};
    const double want[18] = {0.25, 0., 0.75, 1., 1., 1.,   0.5, 0.5, 0.5, 2., 3., 4.,   0.5, 0.5, 0.5, 1., 1., 1.};
    const double want_d[18] = {1., -2., 0.5, 0., 0., 0.,   0., 0., 0., -0.5, 0.25, 8.,   0., 0., 0., 0., 0., 0.};
    std::vector<V3> target((std::size_t)NPIX);
    for (std::size_t i = 0; i < target.size(); ++i)
        target[i] = V3{0.01 * double(i) + 0.1, 0.2, 0.3 - 0.01 * double(i)};       // (not exact in float)
    for (int f64 = 0; f64 < 2; ++f64)
        for (int reuse = 0; reuse < 2; ++reuse)
            for (int mode = 0; mode < 4; ++mode) {        // everything, images alone (no target), sums alone, the tangent images alone
                const bool with_imgs = mode == 0 || mode == 1, with_tans = mode == 0 || mode == 3, with_target = mode == 0 || mode == 2;
                const hip::Options opt = options(f64 != 0, reuse != 0);
                std::vector<V3> imgs((std::size_t)NPIX * 3, V3(-1.)), tans((std::size_t)NPIX * 3, V3(-1.));
                g_calls.clear();
                const hip::SetsAlong<double> r = hip::render_param_sets_along(w.scene, w.cam, w.tracer, 6, sets, with_target ? target.data() : nullptr,
                                                                             with_imgs ? imgs.data() : nullptr, with_tans ? tans.data() : nullptr, opt);
                if (!reuse)
                    CHECK(log_is({"create 3", "upload 3 2", "destroy"}));
                else
                    CHECK(f64 == 0 && mode == 0 ? log_is({"create 3", "upload 3 2"}) : log_is({}));
                CHECK(g_calls.size() == 1);
                const Call& c = g_calls[0];
                CHECK(c.rp.spp == 6 && c.rp.min_bounces == 3 && c.rp.absorb == 0.75 && c.rp.max_depth == 9 && c.rp.seed == 7u && c.rp.shard == 0 &&
                      c.rp.n_shards == 1 && c.rp.band_rows == 5 && c.rp.flags == (f64 ? 0x10u : 0u) && c.rp.batch_paths == 4096 &&
                      c.rp.bounces_per_launch == 2 && c.rp.reserved == 0);
                CHECK(c.cam.width == cd.width && c.cam.height == cd.height && c.cam.vfov == cd.vfov);
                for (int i = 0; i < 3; ++i)
                    CHECK(c.cam.eye[i] == cd.eye[i] && c.cam.forward[i] == cd.forward[i] && c.cam.right[i] == cd.right[i] && c.cam.up[i] == cd.up[i]);
                CHECK(c.n_sets == 3 && !c.sets_null && !c.dirs_null && c.sets.size() == 18 && c.dirs.size() == 18);
                for (int i = 0; i < 18; ++i)
                    CHECK(c.sets[(std::size_t)i] == want[i] && c.dirs[(std::size_t)i] == want_d[i]);      // (handles not listed: direction 0)
                CHECK(c.target_null == !with_target && c.images_null == !with_imgs && c.tangents_null == !with_tans);
                CHECK(c.loss_null == !with_target && c.dloss_null == !with_target && !c.curv_null && !c.stats_null);
                CHECK(r.curvatures.size() == 9);
                for (std::size_t i = 0; i < 9; ++i)
                    CHECK(r.curvatures[i] == pat_curv(i));
                if (with_target) {
                    CHECK(c.target.size() == (std::size_t)NPIX * 3);
                    for (std::size_t i = 0; i < target.size(); ++i)
                        for (int ch = 0; ch < 3; ++ch)
                            CHECK(c.target[i * 3 + (std::size_t)ch] == float(target[i][ch]));
                    CHECK(r.losses.size() == 9 && r.slopes.size() == 9);
                    for (std::size_t i = 0; i < 9; ++i)
                        CHECK(r.losses[i] == pat_loss(i) && r.slopes[i] == pat_dloss(i));
                } else
                    CHECK(r.losses.empty() && r.slopes.empty());
                for (std::size_t i = 0; i < imgs.size(); ++i)
                    for (int ch = 0; ch < 3; ++ch) {
                        CHECK(imgs[i][ch] == (with_imgs ? double(pat_img(i * 3 + (std::size_t)ch)) : -1.));
                        CHECK(tans[i][ch] == (with_tans ? double(pat_tan(i * 3 + (std::size_t)ch)) : -1.));
                    }
                CHECK(r.stats.paths == 11 && r.stats.segments == 22 && r.stats.capped_paths == 33 && r.stats.ms == 44.5);
                // the scene's own values are what they were
                CHECK(w.white[0] == 0.5 && w.white[1] == 0.5 && w.white[2] == 0.5 && w.emission[0] == 1.);
            }
    hip::release_contexts();
    CHECK(log_is({"destroy"}));
    // the exceptions, each with its text; none reaches the library
    g_calls.clear();
    {
        Vector<double, 3, true> stranger(V3(0.25), true);
        const hip::Options opt = options(false, false);
        CHECK(throws_exactly([&] { hip::render_param_sets_along(w.scene, w.cam, w.tracer, 6, {{{stranger, V3(1.), V3(1.)}}}, (const V3*)nullptr, (V3*)nullptr, (V3*)nullptr, opt); },
                             "drt::hip::render_param_sets_along: a listed parameter is not used by the scene"));
        hip::Options bad = opt;
        bad.backward = true;
        CHECK(throws_exactly([&] { hip::render_param_sets_along(w.scene, w.cam, w.tracer, 6, sets, target.data(), (V3*)nullptr, (V3*)nullptr, bad); },
                             "drt::hip::render_param_sets_along: a forward render takes no reverse-mode option (backward, unbiased, sample_loss_l2)"));
        bad = opt;
        bad.sample_loss_l2 = true;
        CHECK(throws_exactly([&] { hip::render_param_sets_along(w.scene, w.cam, w.tracer, 6, sets, target.data(), (V3*)nullptr, (V3*)nullptr, bad); },
                             "drt::hip::render_param_sets_along: a forward render takes no reverse-mode option (backward, unbiased, sample_loss_l2)"));
        bad = opt;
        bad.devices = {3, 4};
        CHECK(throws_exactly([&] { hip::render_param_sets_along(w.scene, w.cam, w.tracer, 6, sets, target.data(), (V3*)nullptr, (V3*)nullptr, bad); },
                             "drt::hip::render_param_sets_along: one device (render shards on plain contexts and add them)"));
        CHECK(g_calls.empty());
        g_log.clear();
        // a refusal of the library arrives as the context's exception, with the library's words
        g_answer = DRT_ERR_UNSUPPORTED;
        bool threw = false;
        try {
            hip::render_param_sets_along(w.scene, w.cam, w.tracer, 6, sets, target.data(), (V3*)nullptr, (V3*)nullptr, opt);
        } catch (const std::runtime_error& e) {
            threw = std::strstr(e.what(), "drt_hip_render_param_sets_along") != nullptr && std::strstr(e.what(), "stub") != nullptr;
            if (!threw)
                std::printf("threw \"%s\"\n", e.what());
        }
        g_answer = DRT_OK;
        CHECK(threw && g_calls.size() == 1);
    }
    return 0;
}

int main()
{
    if (checks())
        return 1;
    std::printf("ok\n");
    return 0;
}
