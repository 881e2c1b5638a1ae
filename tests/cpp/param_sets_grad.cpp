// drt::hip::render_param_sets_grad (include/drt/hip.hpp) against recording stubs of the drt_hip_* functions it reaches, in the style of
// param_sets_along.cpp: libdrt_hip.so is not linked.  The stub keeps the drt_render_params, the camera, the sets, the adjoints and which
// pointers were NULL, and writes a pattern into the gradients; where the gradients land (per set, keyed by the scene's handles), Stats and
// the exceptions' texts are compared with literals: the glue adds nothing to the ABI's results.  Prints "ok" and exits 0, or reports the
// first failure.
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
    bool sets_null = true, adjoints_null = true, grads_null = true, stats_null = true;
    std::vector<double> sets;
    std::vector<float> adjoints;
};
static std::vector<Call> g_calls;
static std::vector<std::string> g_log;

static double pat_grad(std::size_t i) { return 300.25 - 7. * double(i); }
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
int drt_hip_render_param_sets_grad(drt_hip_ctx* ctx, const drt_camera_desc* cam, const drt_render_params* rp, int32_t n_sets,
                                   const double* param_sets, const float* adjoints_rgb, double* out_param_grads, drt_hip_stats* stats)
{
    g_calls.emplace_back();
    Call& c = g_calls.back();
    c.ctx = ctx; c.rp = *rp; c.cam = *cam; c.n_sets = n_sets;
    c.sets_null = !param_sets; c.adjoints_null = !adjoints_rgb; c.grads_null = !out_param_grads; c.stats_null = !stats;
    const std::size_t n = (std::size_t)n_sets * (std::size_t)ctx->n_params * 3;
    if (param_sets)
        c.sets.assign(param_sets, param_sets + n);
    if (adjoints_rgb)
        c.adjoints.assign(adjoints_rgb, adjoints_rgb + (std::size_t)n_sets * floats_of(cam));
    for (std::size_t i = 0; out_param_grads && i < n; ++i)
        out_param_grads[i] = pat_grad(i);
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
    // set 0: white replaced (listed twice: the last value stands), the emission as in the scene; set 1: the emission alone; set 2: empty --
    // the scene's values
    const std::vector<hip::ParamSet<double>> sets = {
        {{w.white, V3{0.1, 0.2, 0.3}}, {w.white, V3{0.25, 0., 0.75}}},
        {{w.emission, V3{2., 3., 4.}}},
        {}};
    const double want[18] = {0.25, 0., 0.75, 1., 1., 1.,   0.5, 0.5, 0.5, 2., 3., 4.,   0.5, 0.5, 0.5, 1., 1., 1.};
    std::vector<V3> adjoints((std::size_t)NPIX * 3);
    for (std::size_t i = 0; i < adjoints.size(); ++i)
        adjoints[i] = V3{0.01 * double(i) + 0.1, -0.2, 0.3 - 0.01 * double(i)};       // (not exact in float)
    for (int f64 = 0; f64 < 2; ++f64)
        for (int reuse = 0; reuse < 2; ++reuse)
            for (int mode = 0; mode < 3; ++mode) {        // with adjoints, without, with adjoints and Options::backward (implied: the same call)
                const bool with_adj = mode != 1;
                hip::Options opt = options(f64 != 0, reuse != 0);
                opt.backward = mode == 2;
                g_calls.clear();
                const hip::SetsGrad<double> r = hip::render_param_sets_grad(w.scene, w.cam, w.tracer, 6, sets, with_adj ? adjoints.data() : nullptr, opt);
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
                CHECK(c.n_sets == 3 && !c.sets_null && c.sets.size() == 18 && !c.grads_null && !c.stats_null);
                for (int i = 0; i < 18; ++i)
                    CHECK(c.sets[(std::size_t)i] == want[i]);      // (handles not listed: the scene's value)
                CHECK(c.adjoints_null == !with_adj);
                if (with_adj) {
                    CHECK(c.adjoints.size() == (std::size_t)NPIX * 9);
                    for (std::size_t i = 0; i < adjoints.size(); ++i)
                        for (int ch = 0; ch < 3; ++ch)
                            CHECK(c.adjoints[i * 3 + (std::size_t)ch] == float(adjoints[i][ch]));
                }
                // where the gradients land: per set, every parameter of the scene in the scene's order, keyed by its handle
                CHECK(r.grads.size() == 3);
                for (std::size_t k = 0; k < 3; ++k) {
                    CHECK(r.grads[k].size() == 2);
                    CHECK(r.grads[k][0].first.id() == w.white.id() && r.grads[k][1].first.id() == w.emission.id());
                    for (std::size_t p = 0; p < 2; ++p)
                        for (int ch = 0; ch < 3; ++ch)
                            CHECK(r.grads[k][p].second[ch] == pat_grad((k * 2 + p) * 3 + (std::size_t)ch));
                }
                CHECK(r.stats.paths == 11 && r.stats.segments == 22 && r.stats.capped_paths == 33 && r.stats.ms == 44.5);
                // the scene's own values and gradients are what they were
                CHECK(w.white[0] == 0.5 && w.white[1] == 0.5 && w.white[2] == 0.5 && w.emission[0] == 1.);
                CHECK(w.white.grad()[0] == 0. && w.white.grad()[1] == 0. && w.white.grad()[2] == 0.);
            }
    hip::release_contexts();
    CHECK(log_is({"destroy"}));
    // the exceptions, each with its text; none reaches the library
    g_calls.clear();
    {
        Vector<double, 3, true> stranger(V3(0.25), true);
        const hip::Options opt = options(false, false);
        CHECK(throws_exactly([&] { hip::render_param_sets_grad(w.scene, w.cam, w.tracer, 6, {{{stranger, V3(1.)}}}, (const V3*)nullptr, opt); },
                             "drt::hip::render_param_sets_grad: a listed parameter is not used by the scene"));
        hip::Options bad = opt;
        bad.unbiased = true;
        CHECK(throws_exactly([&] { hip::render_param_sets_grad(w.scene, w.cam, w.tracer, 6, sets, adjoints.data(), bad); },
                             "drt::hip::render_param_sets_grad: the biased operator's summed gradients (backward is implied; no unbiased, no sample_loss_l2)"));
        bad = opt;
        bad.sample_loss_l2 = true;
        CHECK(throws_exactly([&] { hip::render_param_sets_grad(w.scene, w.cam, w.tracer, 6, sets, adjoints.data(), bad); },
                             "drt::hip::render_param_sets_grad: the biased operator's summed gradients (backward is implied; no unbiased, no sample_loss_l2)"));
        bad = opt;
        bad.devices = {3, 4};
        CHECK(throws_exactly([&] { hip::render_param_sets_grad(w.scene, w.cam, w.tracer, 6, sets, adjoints.data(), bad); },
                             "drt::hip::render_param_sets_grad: one device (render shards on plain contexts and add them)"));
        CHECK(g_calls.empty());
        g_log.clear();
        // a refusal of the library arrives as the context's exception, with the library's words
        g_answer = DRT_ERR_UNSUPPORTED;
        bool threw = false;
        try {
            hip::render_param_sets_grad(w.scene, w.cam, w.tracer, 6, sets, adjoints.data(), opt);
        } catch (const std::runtime_error& e) {
            threw = std::strstr(e.what(), "drt_hip_render_param_sets_grad") != nullptr && std::strstr(e.what(), "stub") != nullptr;
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
