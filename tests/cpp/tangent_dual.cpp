// Forward mode through the host API (drt::hip::render_tangent, drt::hip::render on a Scene<Dual<double>>).
//   tangent_dual flatten   no device: a Dual scene flattens into real parts (the parameters) and dual parts (the direction); a dual
//                          part where the device does not differentiate, a reverse-mode option, an unused handle: all throw
//   tangent_dual device    drt::hip::render<Dual<double>> in the f64 mode against the host API's own per-ray loop on Dual numbers
//                          (the loop of dual_end_to_end.cpp, on the device's per-path streams): 1e-9 per pixel, real and dual parts
// Prints "ok ..." and exits 0, or reports the first failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <tuple>
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
using D = Dual<double>;
using DV = Vector<D, 3>;
using DP = Vector<D, 3, true>;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

// the reference's scene (render.cpp:26-59) on Dual numbers; every parameter carries a direction, red's zero channels included
struct Room {
    DP red{DV{D(0.5, 0.7), D(0., -0.4), D(0., 0.9)}, true}, green{DV{D(0., 0.3), D(0.5, -0.6), D(0., 0.5)}, true};
    DP white{DV{D(0.5, -0.8), D(0.5, 0.45), D(0.5, 0.35)}, true}, emission{DV{D(1., 0.6), D(1., -0.7), D(1., 0.25)}, true};
    std::shared_ptr<BxDF<D>> dred = std::make_shared<DiffuseBxDF<D>>(red), dgreen = std::make_shared<DiffuseBxDF<D>>(green),
                             dwhite = std::make_shared<DiffuseBxDF<D>>(white), spec = std::make_shared<SpecularBxDF<D>>(white, 30);
    std::shared_ptr<Emitter<D>> emitter = std::make_shared<AreaEmitter<D>>(emission);
    Sphere<D> s1{DV{0., 0., 3.}, 1., spec}, s2{DV{-1., 1., 4.5}, 1., dwhite};
    Plane<D> p1{DV{-1., 0., 0.}, -3., dred}, p2{DV{1., 0., 0.1}, -3., dgreen}, p3{DV{0., 0., -1.}, -6., dwhite}, p4{DV{0, 0, 1}, 0, dwhite},
        p5{DV{0., 1., 0.}, -3., dwhite}, p6{DV{0., -1., 0.}, -3., dwhite};
    Sphere<D> light{DV{0., 3., 3.}, 1., nullptr, emitter};
    Scene<D> scene() { return Scene<D>{&s1, &s2, &p1, &p2, &p3, &p4, &p5, &p6, &light}; }
};

template <typename F>
static bool throws_with(F&& f, const char* word)
{
    try {
        f();
    } catch (const std::runtime_error& e) {
        if (std::strstr(e.what(), word))
            return true;
        std::printf("threw \"%s\", not about \"%s\"\n", e.what(), word);
        return false;
    }
    std::printf("did not throw (expected \"%s\")\n", word);
    return false;
}

static int flatten_checks()
{
    Room room;
    Scene<D> scene = room.scene();
    std::vector<double> v;
    hip::FlatScene<D> flat = hip::flatten_dual(scene, v);
    // parameters in order of first use: white (the front sphere's lobe), red, green, emission
    const DP* order[4] = {&room.white, &room.red, &room.green, &room.emission};
    CHECK(flat.handles.size() == 4 && flat.params.size() == 12 && v.size() == 12);
    for (int p = 0; p < 4; ++p)
        for (int c = 0; c < 3; ++c) {
            CHECK(flat.handles[p].id() == order[p]->id());
            CHECK(flat.params[p * 3 + c] == (*order[p])[c].real());
            CHECK(v[p * 3 + c] == (*order[p])[c].dual());
        }
    CHECK(v[1 * 3 + 1] == -0.4 && flat.params[1 * 3 + 1] == 0.);      // red.g: a zero channel with a direction
    std::vector<DV> img(4 * 3);
    Camera<D> cam(4, 3);
    cam.look_at(DV{0, 0, 0}, DV{0, 0, 1});
    Pathtracer<D> tracer(0.3, 2);
    // a dual part where the device does not differentiate: named, never dropped
    {
        Sphere<D> moved(DV{D(0., 1.), 0., 3.}, 1., room.dwhite);
        Scene<D> s2 = scene;
        s2.push_back(&moved);
        CHECK(throws_with([&] { hip::flatten_dual(s2, v); }, "centre"));
        CHECK(throws_with([&] { hip::render(s2, cam, tracer, 1, img.data()); }, "centre"));
        Plane<D> tilted(DV{0., D(1., 0.5), 0.}, -3., room.dwhite);
        Scene<D> s3 = scene;
        s3.push_back(&tilted);
        CHECK(throws_with([&] { hip::flatten_dual(s3, v); }, "normal"));
    }
    {
        Camera<D> dcam(4, 3);
        dcam.look_at(DV{D(0., 1e-3), 0, 0}, DV{0, 0, 1});
        CHECK(throws_with([&] { hip::describe_dual(dcam); }, "camera"));
        CHECK(throws_with([&] { hip::render(scene, dcam, tracer, 1, img.data()); }, "camera"));
    }
    // reverse-mode notions together with Dual
    {
        hip::Options opt;
        opt.backward = true;
        CHECK(throws_with([&] { hip::render(scene, cam, tracer, 1, img.data(), opt); }, "reverse-mode"));
        hip::Options opt2;
        opt2.sample_loss_l2 = true;
        CHECK(throws_with([&] { hip::render(scene, cam, tracer, 1, img.data(), opt2); }, "reverse-mode"));
        CHECK(throws_with([&] { hip::render(scene, cam, tracer, 1, img.data(), hip::Options(), img.data()); }, "adjoint"));
    }
    // render_tangent: a listed handle the scene does not use
    {
        using T = double;
        Vector<T, 3, true> albedo(Vector<T, 3>(0.5), true), stranger(Vector<T, 3>(0.25), true), emission(Vector<T, 3>(1.), true);
        auto mat = std::make_shared<DiffuseBxDF<T>>(albedo);
        auto em = std::make_shared<AreaEmitter<T>>(emission);
        Sphere<T> ball(Vector<T, 3>{0., 0., 3.}, 1., mat), light(Vector<T, 3>{0., 3., 3.}, 1., nullptr, em);
        Scene<T> s{&ball, &light};
        Camera<T> c(4, 3);
        Pathtracer<T> tr(1.0, 2);
        std::vector<Vector<T, 3>> a(12), b(12);
        CHECK(throws_with([&] { hip::render_tangent(s, c, tr, 1, {{stranger, Vector<T, 3>(1.)}}, a.data(), b.data()); }, "not used by the scene"));
        hip::Options opt;
        opt.unbiased = true;
        CHECK(throws_with([&] { hip::render_tangent(s, c, tr, 1, {{albedo, Vector<T, 3>(1.)}}, a.data(), b.data(), opt); }, "reverse-mode"));
    }
    std::printf("ok\n");
    return 0;
}

static int device_checks()
{
    int bad = 0;
    double worst_all = 0;
    struct Case { double absorb; std::size_t min_bounces; } cases[2] = {{1.0, 5}, {0.5, 1}};       // lockstep, regenerating
    for (const Case& cs : cases) {
        Room room;
        Scene<D> scene = room.scene();
        const std::size_t W = 24, H = 18, spp = 4;
        Camera<D> cam(W, H);
        cam.look_at(DV{0, 0, 0}, DV{0, 0, 1});
        Pathtracer<D> tracer(cs.absorb, cs.min_bounces);
        // the host API's own loop on Dual numbers (dual_end_to_end.cpp), on the device's per-path streams
        std::vector<DV> cpu(W * H, DV(D(0.)));
        for (std::size_t y = 0; y < H; ++y)
            for (std::size_t x = 0; x < W; ++x)
                for (std::size_t i = 0; i < spp; ++i) {
                    random::begin_path(11u, (uint64_t)(y * W + x) * spp + i);
                    DV dir;
                    double pdf;
                    std::tie(dir, pdf) = cam.sample(x, y);
                    auto radiance = tracer.trace(scene, cam.eye(), dir);
                    for (int c = 0; c < 3; ++c)
                        cpu[y * W + x][c] += detach(radiance)[c] / (pdf * double(spp));
                }
        random::use_libc();
        std::vector<DV> dev(W * H, DV(D(0.)));
        hip::Options opt;
        opt.f64 = true;
        opt.seed = 11;
        const hip::Stats st = hip::render(scene, cam, tracer, spp, dev.data(), opt);
        double re_scale = 0, du_scale = 0, re_worst = 0, du_worst = 0;
        for (std::size_t i = 0; i < W * H; ++i)
            for (int c = 0; c < 3; ++c) {
                re_scale = std::fmax(re_scale, std::fabs(cpu[i][c].real()));
                du_scale = std::fmax(du_scale, std::fabs(cpu[i][c].dual()));
                re_worst = std::fmax(re_worst, std::fabs(dev[i][c].real() - cpu[i][c].real()));
                du_worst = std::fmax(du_worst, std::fabs(dev[i][c].dual() - cpu[i][c].dual()));
            }
        std::printf("absorb %.1f from bounce %zu: real %.3g of %.3g, dual %.3g of %.3g (%llu segments)\n", cs.absorb, cs.min_bounces, re_worst,
                    re_scale, du_worst, du_scale, st.segments);
        if (!(re_scale > 0 && du_scale > 0 && re_worst <= 1e-9 * re_scale && du_worst <= 1e-9 * du_scale))
            ++bad;
        worst_all = std::fmax(worst_all, std::fmax(re_worst / re_scale, du_worst / du_scale));
    }
    // render_tangent for T = double: the same direction as (handle, direction) pairs gives the Dual render's dual parts
    {
        using T = double;
        Vector<T, 3, true> albedo(Vector<T, 3>{0.6, 0., 0.4}, true), emission(Vector<T, 3>(1.), true);
        Vector<D, 3, true> dalbedo(DV{D(0.6, 0.5), D(0., -1.), D(0.4, 2.)}, true), demission(DV{D(1., 0.), D(1., 1.5), D(1., 0.)}, true);
        auto mat = std::make_shared<DiffuseBxDF<T>>(albedo);
        auto em = std::make_shared<AreaEmitter<T>>(emission);
        auto dmat = std::make_shared<DiffuseBxDF<D>>(dalbedo);
        auto dem = std::make_shared<AreaEmitter<D>>(demission);
        Sphere<T> ball(Vector<T, 3>{0., 0., 3.}, 1., mat), light(Vector<T, 3>{0., 3., 3.}, 1., nullptr, em);
        Plane<T> floor_(Vector<T, 3>{0., 1., 0.}, -3., mat);
        Sphere<D> dball(DV{0., 0., 3.}, 1., dmat), dlight(DV{0., 3., 3.}, 1., nullptr, dem);
        Plane<D> dfloor(DV{0., 1., 0.}, -3., dmat);
        Scene<T> s{&ball, &floor_, &light};
        Scene<D> ds{&dball, &dfloor, &dlight};
        Camera<T> c(20, 16);
        c.look_at(Vector<T, 3>{0, 0, 0}, Vector<T, 3>{0, 0, 1});
        Camera<D> dc(20, 16);
        dc.look_at(DV{0, 0, 0}, DV{0, 0, 1});
        Pathtracer<T> tr(1.0, 4);
        Pathtracer<D> dtr(1.0, 4);
        hip::Options opt;
        opt.f64 = true;
        std::vector<Vector<T, 3>> a(320), b(320);
        std::vector<DV> d(320);
        hip::render_tangent(s, c, tr, 3, {{albedo, Vector<T, 3>{0.5, -1., 2.}}, {emission, Vector<T, 3>{0., 1.5, 0.}}}, a.data(), b.data(), opt);
        hip::render(ds, dc, dtr, 3, d.data(), opt);
        double any = 0;
        for (int i = 0; i < 320; ++i)
            for (int ch = 0; ch < 3; ++ch) {
                bad += (a[i][ch] != d[i][ch].real()) + (b[i][ch] != d[i][ch].dual());
                any = std::fmax(any, std::fabs(b[i][ch]));
            }
        bad += !(any > 0);
    }
    hip::release_contexts();
    if (bad) {
        std::printf("FAILED (%d)\n", bad);
        return 1;
    }
    std::printf("ok %.3g\n", worst_all);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "device")
        return device_checks();
    return flatten_checks();
}
