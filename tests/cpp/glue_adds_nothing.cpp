// The host glue (include/drt/hip.hpp) adds nothing to what the library computes: every entry point of drt::hip against the
// drt_hip_* function underneath it, called directly on a context of this program's own with flatten(scene).desc(), describe(cam)
// and the same render parameters -- images, gradient image, tangent images, gradients, A, b, loss, segment and path counts equal
// BIT FOR BIT (the renders are repeatable to the bit: test_host_api.py's frames-in-flight and dropped-frame tests).
// 48 x 32 x 4 spp: several waves, a partial last one (1536 pixels), both parameter roles (a colour, an emission).
// Prints "bad 0" and exits 0, or a line per entry point that differs.
#include <cstdio>
#include <memory>
#include <vector>

#include "drt/hip.hpp"

using namespace drt;
using T = double;
using V3 = Vector<T, 3>;

static const std::size_t W = 48, H = 32, NPIX = W * H, SPP = 4;

static drt_render_params params(uint32_t flags)
{
    drt_render_params rp{};
    rp.spp = (int32_t)SPP;
    rp.min_bounces = 4;
    rp.absorb = 1.0;
    rp.seed = 1;
    rp.n_shards = 1;
    rp.band_rows = 16;
    rp.flags = flags;
    return rp;
}

template <typename F>
static int differing(const std::vector<V3>& glue, const std::vector<F>& direct)
{
    int bad = 0;
    for (std::size_t i = 0; i < NPIX; ++i)
        for (int c = 0; c < 3; ++c)
            bad += glue[i][c] != T(direct[i * 3 + c]);
    return bad;
}

static int report(const char* what, int bad)
{
    if (bad)
        std::printf("%s: %d values differ\n", what, bad);
    return bad;
}

int main()
{
    Vector<T, 3, true> white(V3{0.5, 0.5, 0.5}, true), emission(V3(1), true);
    auto mat = std::make_shared<DiffuseBxDF<T>>(white);
    auto em = std::make_shared<AreaEmitter<T>>(emission);
    Sphere<T> ball(V3{0., 0., 3.}, 1., mat);
    Plane<T> floor_(V3{0., 1., 0.}, -3., mat);
    Sphere<T> light(V3{0., 3., 3.}, 1., nullptr, em);
    Scene<T> scene{&ball, &floor_, &light};
    Camera<T> cam(W, H);
    cam.look_at(V3{0, 0, 0}, V3{0, 0, 1});
    Pathtracer<T> tracer(1.0, 4);

    // the library, directly
    const hip::FlatScene<T> flat = hip::flatten(scene);
    const drt_scene_desc sd = flat.desc();
    const drt_camera_desc cd = hip::describe(cam);
    hip::Context ctx(0);
    ctx.check(drt_hip_upload_scene(ctx.get(), &sd), "drt_hip_upload_scene");
    if (flat.handles.size() != 2 || flat.handles[0].id() != white.id() || flat.handles[1].id() != emission.id()) {
        std::printf("unexpected parameter order\n");
        return 1;
    }

    hip::Options opt;
    opt.reuse_context = false;
    int bad = 0;
    auto grads_differ = [&](const std::vector<double>& direct) {
        int n = 0;
        for (int c = 0; c < 3; ++c)
            n += (white.grad()[c] != direct[(std::size_t)c]) + (emission.grad()[c] != direct[3 + (std::size_t)c]);
        white.grad() = V3(0.);
        emission.grad() = V3(0.);
        return n;
    };
    auto counts_differ = [](const hip::Stats& a, const drt_hip_stats& b) {
        return (a.paths != b.paths) + (a.segments != b.segments) + (a.capped_paths != b.capped_paths) + (a.segments == 0);
    };

    // render, backward
    std::vector<V3> first(NPIX);
    {
        hip::Options o = opt;
        o.backward = true;
        const hip::Stats st = hip::render(scene, cam, tracer, SPP, first.data(), o);
        const drt_render_params rp = params(DRT_RENDER_BACKWARD);
        std::vector<float> rgb(NPIX * 3);
        std::vector<double> g(6);
        drt_hip_stats ds{};
        ctx.check(drt_hip_render(ctx.get(), &cd, &rp, nullptr, rgb.data(), g.data(), &ds), "drt_hip_render");
        bad += report("render: image", differing(first, rgb));
        bad += report("render: gradients", grads_differ(g));
        bad += report("render: counts", counts_differ(st, ds));
    }
    // submit + get, backward, with an adjoint image
    {
        hip::Options o = opt;
        o.backward = true;
        std::vector<V3> img(NPIX), adjoint(NPIX);
        std::vector<float> adj(NPIX * 3);
        for (std::size_t i = 0; i < NPIX; ++i)
            for (int c = 0; c < 3; ++c) {
                adjoint[i][c] = 0.25 + 0.001 * double(i % 97) + 0.1 * c;
                adj[i * 3 + c] = float(adjoint[i][c]);
            }
        hip::Pending<T> p = hip::submit(scene, cam, tracer, SPP, img.data(), o, adjoint.data());
        const hip::Stats st = p.get();
        const drt_render_params rp = params(DRT_RENDER_BACKWARD);
        std::vector<float> rgb(NPIX * 3);
        std::vector<double> g(6);
        drt_hip_stats ds{};
        uint64_t ticket = 0;
        ctx.check(drt_hip_render_async(ctx.get(), &cd, &rp, adj.data(), rgb.data(), g.data(), &ticket), "drt_hip_render_async");
        ctx.check(drt_hip_wait(ctx.get(), ticket, &ds), "drt_hip_wait");
        bad += report("submit: image", differing(img, rgb));
        bad += report("submit: gradients", grads_differ(g));
        bad += report("submit: counts", counts_differ(st, ds));
    }
    // the gradient image of either parameter
    for (int index = 0; index < 2; ++index) {
        std::vector<V3> img(NPIX), gimg(NPIX);
        const hip::Stats st = hip::render_gradient_image(scene, cam, tracer, SPP, index ? emission : white, img.data(), gimg.data(), opt);
        const drt_render_params rp = params(0);
        std::vector<float> rgb(NPIX * 3), grgb(NPIX * 3);
        drt_hip_stats ds{};
        ctx.check(drt_hip_render_gradient_image(ctx.get(), &cd, &rp, index, nullptr, rgb.data(), grgb.data(), &ds), "drt_hip_render_gradient_image");
        bad += report("render_gradient_image: image", differing(img, rgb));
        bad += report("render_gradient_image: gradient image", differing(gimg, grgb));
        bad += report("render_gradient_image: counts", counts_differ(st, ds));
    }
    // the tangent image, f32 and f64
    for (int f64 = 0; f64 < 2; ++f64) {
        hip::Options o = opt;
        o.f64 = f64 != 0;
        std::vector<V3> img(NPIX), timg(NPIX);
        const hip::Stats st = hip::render_tangent(scene, cam, tracer, SPP, {{white, V3{0.5, -1., 2.}}, {emission, V3{0., 1.5, 0.25}}}, img.data(), timg.data(), o);
        const drt_render_params rp = params(f64 ? DRT_RENDER_F64 : 0u);
        const double v[6] = {0.5, -1., 2., 0., 1.5, 0.25};
        drt_hip_stats ds{};
        if (f64) {
            std::vector<double> rgb(NPIX * 3), trgb(NPIX * 3);
            ctx.check(drt_hip_render_tangent_double(ctx.get(), &cd, &rp, v, rgb.data(), trgb.data(), &ds), "drt_hip_render_tangent_double");
            bad += report("render_tangent f64: image", differing(img, rgb));
            bad += report("render_tangent f64: tangent image", differing(timg, trgb));
        } else {
            std::vector<float> rgb(NPIX * 3), trgb(NPIX * 3);
            ctx.check(drt_hip_render_tangent(ctx.get(), &cd, &rp, v, rgb.data(), trgb.data(), &ds), "drt_hip_render_tangent");
            bad += report("render_tangent f32: image", differing(img, rgb));
            bad += report("render_tangent f32: tangent image", differing(timg, trgb));
        }
        bad += report("render_tangent: counts", counts_differ(st, ds));
    }
    // the normal equations against a target: the first render's image, dimmed
    {
        std::vector<V3> target(NPIX), img(NPIX);
        std::vector<float> tgt(NPIX * 3);
        for (std::size_t i = 0; i < NPIX; ++i)
            for (int c = 0; c < 3; ++c) {
                target[i][c] = 0.75 * first[i][c];
                tgt[i * 3 + c] = float(target[i][c]);
            }
        const hip::NormalEquations<T> ne = hip::normal_equations(scene, cam, tracer, SPP, opt, hip::TargetOrResidual<T>::target(target.data()), img.data());
        const drt_render_params rp = params(0);
        std::vector<float> rgb(NPIX * 3);
        std::vector<double> A(12), b(6), loss(3);
        drt_hip_stats ds{};
        ctx.check(drt_hip_render_normal_equations(ctx.get(), &cd, &rp, tgt.data(), nullptr, rgb.data(), A.data(), b.data(), loss.data(), nullptr, &ds),
                  "drt_hip_render_normal_equations");
        bad += report("normal_equations: image", differing(img, rgb));
        bad += report("normal_equations: A", (ne.A != A) + (ne.A.size() != 12) + (A[0] == 0.));
        bad += report("normal_equations: b", (ne.b != b) + (ne.b.size() != 6));
        bad += report("normal_equations: loss", (ne.loss != loss) + (ne.loss.size() != 3) + (loss[0] == 0.));
        bad += report("normal_equations: counts", counts_differ(ne.stats, ds));
    }
    std::printf("bad %d\n", bad);
    hip::release_contexts();
    return bad ? 1 : 0;
}
