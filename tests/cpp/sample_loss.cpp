// The per-sample loss through the host API (drt::hip::render_sample_loss).
//   sample_loss flatten   no device: the options that make no sense, a missing target, too many values -- all throw before a device is asked for
//   sample_loss device    drt::hip::render_sample_loss in the f64 mode against the host API's own loop -- begin_path, trace,
//                         radiance.backward(grad(detach(radiance), target)), the loss added in double -- on the device's per-path streams:
//                         1e-9 on every handle's gradient, 1e-12 on the loss, both tracers
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
#include "drt/emitter.hpp"
#include "drt/hip.hpp"
#include "drt/pathtracer.hpp"
#include "drt/shape.hpp"
#include "drt/vector.hpp"

using namespace drt;
using T = double;
using V = Vector<T, 3>;
using P = Vector<T, 3, true>;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

// the reference's scene (render.cpp:26-59), the Room of tangent_dual.cpp on plain doubles
struct Room {
    P red{V{0.5, 0., 0.}, true}, green{V{0., 0.5, 0.}, true}, white{V{0.5, 0.5, 0.5}, true}, emission{V{1., 1., 1.}, true};
    std::shared_ptr<BxDF<T>> dred = std::make_shared<DiffuseBxDF<T>>(red), dgreen = std::make_shared<DiffuseBxDF<T>>(green),
                             dwhite = std::make_shared<DiffuseBxDF<T>>(white), spec = std::make_shared<SpecularBxDF<T>>(white, 30);
    std::shared_ptr<Emitter<T>> emitter = std::make_shared<AreaEmitter<T>>(emission);
    Sphere<T> s1{V{0., 0., 3.}, 1., spec}, s2{V{-1., 1., 4.5}, 1., dwhite};
    Plane<T> p1{V{-1., 0., 0.}, -3., dred}, p2{V{1., 0., 0.1}, -3., dgreen}, p3{V{0., 0., -1.}, -6., dwhite}, p4{V{0, 0, 1}, 0, dwhite},
        p5{V{0., 1., 0.}, -3., dwhite}, p6{V{0., -1., 0.}, -3., dwhite};
    Sphere<T> light{V{0., 3., 3.}, 1., nullptr, emitter};
    Scene<T> scene() { return Scene<T>{&s1, &s2, &p1, &p2, &p3, &p4, &p5, &p6, &light}; }
    P* handles[4] = {&red, &green, &white, &emission};
};

// pseudo-Huber, delta = q[0]: per channel delta^2 (sqrt(1 + (d / delta)^2) - 1), d = L - t
static const char* HUBER_SRC =
    "    const R dl = q[0], i2 = div_r(R(1), dl * dl);\n"
    "    const V3<R> d = L - t;\n"
    "    const R sx = sqrt_r(R(1) + d.x * d.x * i2), sy = sqrt_r(R(1) + d.y * d.y * i2), sz = sqrt_r(R(1) + d.z * d.z * i2);\n"
    "    value = dl * dl * ((sx - R(1)) + (sy - R(1)) + (sz - R(1)));\n"
    "    grad = mk<R>(div_r(d.x, sx), div_r(d.y, sy), div_r(d.z, sz));\n";

static double huber(const V& L, const V& t, double delta, V& grad)
{
    double value = 0;
    for (int c = 0; c < 3; ++c) {
        const double d = L[c] - t[c], s = std::sqrt(1.0 + d * d / (delta * delta));
        value += delta * delta * (s - 1.0);
        grad[c] = d / s;
    }
    return value;
}

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
    Scene<T> scene = room.scene();
    Camera<T> cam(4, 3);
    cam.look_at(V{0, 0, 0}, V{0, 0, 1});
    Pathtracer<T> tracer(0.3, 2);
    std::vector<V> img(12), target(12, V(0.25));
    const hip::SampleLoss loss{"pseudo_huber", HUBER_SRC, {0.3}};
    hip::Options unbiased;
    unbiased.unbiased = true;
    CHECK(throws_with([&] { hip::render_sample_loss(scene, cam, tracer, 1, target.data(), img.data(), loss, unbiased); }, "unbiased"));
    hip::Options l2;
    l2.sample_loss_l2 = true;
    CHECK(throws_with([&] { hip::render_sample_loss(scene, cam, tracer, 1, target.data(), img.data(), loss, l2); }, "sample_loss_l2"));
    hip::Options two;
    two.devices = {0, 1};
    CHECK(throws_with([&] { hip::render_sample_loss(scene, cam, tracer, 1, target.data(), img.data(), loss, two); }, "one device"));
    CHECK(throws_with([&] { hip::render_sample_loss(scene, cam, tracer, 1, (const V*)nullptr, img.data(), loss); }, "target"));
    const hip::SampleLoss five{"five", HUBER_SRC, {1, 2, 3, 4, 5}};
    CHECK(throws_with([&] { hip::render_sample_loss(scene, cam, tracer, 1, target.data(), img.data(), five); }, "DRT_MAX_LOSS_VALUES"));
    for (P* h : room.handles)
        for (int c = 0; c < 3; ++c)
            CHECK(h->grad()[c] == 0.);                       // nothing was rendered
    std::printf("ok\n");
    return 0;
}

static int device_checks()
{
    int bad = 0;
    double worst_grad = 0, worst_loss = 0;
    const double delta = 0.3;
    struct Case { double absorb; std::size_t min_bounces; } cases[2] = {{1.0, 4}, {0.5, 1}};       // lockstep, regenerating
    for (const Case& cs : cases) {
        const std::size_t W = 24, H = 18, spp = 4;
        Camera<T> cam(W, H);
        cam.look_at(V{0, 0, 0}, V{0, 0, 1});
        Pathtracer<T> tracer(cs.absorb, cs.min_bounces);
        std::vector<V> target(W * H);
        for (std::size_t i = 0; i < W * H; ++i)
            for (int c = 0; c < 3; ++c)
                target[i][c] = (double)(float)(0.6 * (double)((i * 3 + c) * 2654435761u % 1000u) / 1000.0);   // (float values: the device takes a float image)
        // the host API's own loop, on the device's per-path streams
        Room host;
        Scene<T> hscene = host.scene();
        double host_loss = 0;
        for (std::size_t y = 0; y < H; ++y)
            for (std::size_t x = 0; x < W; ++x)
                for (std::size_t i = 0; i < spp; ++i) {
                    random::begin_path(11u, (uint64_t)(y * W + x) * spp + i);
                    V dir;
                    double pdf;
                    std::tie(dir, pdf) = cam.sample(x, y);
                    auto radiance = tracer.trace(hscene, cam.eye(), dir);
                    V g;
                    host_loss += huber(detach(radiance), target[y * W + x], delta, g);
                    backward(radiance, g);
                }
        random::use_libc();
        Room dev;
        Scene<T> dscene = dev.scene();
        hip::Options opt;
        opt.f64 = true;
        opt.seed = 11;
        std::vector<V> img(W * H);
        const hip::SampleLossResult r = hip::render_sample_loss(dscene, cam, tracer, spp, target.data(), img.data(), hip::SampleLoss{"pseudo_huber", HUBER_SRC, {delta}}, opt);
        double scale = 0, worst = 0;
        for (int p = 0; p < 4; ++p)
            for (int c = 0; c < 3; ++c) {
                scale = std::fmax(scale, std::fabs(host.handles[p]->grad()[c]));
                worst = std::fmax(worst, std::fabs(dev.handles[p]->grad()[c] - host.handles[p]->grad()[c]));
            }
        const double loss_err = std::fabs(r.loss - host_loss) / host_loss;
        std::printf("absorb %.1f from bounce %zu: gradients %.3g of %.3g, loss %.17g against %.17g (%.3g), %llu segments\n", cs.absorb, cs.min_bounces,
                    worst, scale, r.loss, host_loss, loss_err, r.stats.segments);
        if (!(scale > 0 && host_loss > 0 && worst <= 1e-9 * scale && loss_err <= 1e-12))
            ++bad;
        worst_grad = std::fmax(worst_grad, worst / scale);
        worst_loss = std::fmax(worst_loss, loss_err);
    }
    hip::release_contexts();
    if (bad) {
        std::printf("FAILED (%d)\n", bad);
        return 1;
    }
    std::printf("ok %.3g %.3g\n", worst_grad, worst_loss);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "device")
        return device_checks();
    return flatten_checks();
}
