// A caller's batch of pixels from several cameras through the host API (drt::hip::render_pixels).
//   pixels flatten   no device: what the call refuses before it reaches a context -- no camera, too many, a list count that is not the
//                    cameras', a seed count that is not, cameras of different sizes, an empty batch, a pixel outside the frame, reverse-mode
//                    options it does not take, several devices, nothing to compute
//   pixels device    drt::hip::render_pixels in the f64 mode against the host API's own per-ray loop over the listed pixels on the
//                    device's per-path streams, each entry with its own adjoint (1e-9 of the largest value; the radiance leaves the
//                    library as float)
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
using Vec3 = Vector<T, 3>;
using Var3 = Vector<T, 3, true>;
using Lists = std::vector<std::vector<uint32_t>>;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

// the reference's scene (render.cpp:26-59)
struct Room {
    Var3 red{Vec3{0.5, 0., 0.}, true}, green{Vec3{0., 0.5, 0.}, true}, white{Vec3(0.5), true}, emission{Vec3(1.), true};
    std::shared_ptr<BxDF<T>> dred = std::make_shared<DiffuseBxDF<T>>(red), dgreen = std::make_shared<DiffuseBxDF<T>>(green),
                             dwhite = std::make_shared<DiffuseBxDF<T>>(white);
    std::shared_ptr<Emitter<T>> emitter = std::make_shared<AreaEmitter<T>>(emission);
    Sphere<T> s1{Vec3{0., 0., 3.}, 1., dwhite}, s2{Vec3{-1., 1., 4.5}, 1., dwhite};
    Plane<T> p1{Vec3{-1., 0., 0.}, -3., dred}, p2{Vec3{1., 0., 0.1}, -3., dgreen}, p3{Vec3{0., 0., -1.}, -6., dwhite}, p4{Vec3{0, 0, 1}, 0, dwhite},
        p5{Vec3{0., 1., 0.}, -3., dwhite}, p6{Vec3{0., -1., 0.}, -3., dwhite};
    Sphere<T> light{Vec3{0., 3., 3.}, 1., nullptr, emitter};
    Scene<T> scene() { return Scene<T>{&s1, &s2, &p1, &p2, &p3, &p4, &p5, &p6, &light}; }
    std::vector<Var3*> params() { return {&red, &green, &white, &emission}; }
};

static std::vector<Camera<T>> three_cameras(std::size_t W, std::size_t H)
{
    std::vector<Camera<T>> cams(3, Camera<T>(W, H));
    cams[0].look_at(Vec3{0., 0., 0.}, Vec3{0., 0., 1.});
    cams[1].look_at(Vec3{0.4, -0.2, 0.1}, Vec3{-0.2, 0.1, 1.});
    cams[2].look_at(Vec3{-0.5, 0.3, 0.2}, Vec3{0.3, -0.3, 1.});
    return cams;
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
    Pathtracer<T> tracer(1.0, 3);
    std::vector<Camera<T>> cams = three_cameras(4, 3);
    const Lists lists = {{0u, 5u, 11u}, {}, {7u, 7u}};
    std::vector<Vec3> out(5);
    CHECK(throws_with([&] { hip::render_pixels(scene, std::vector<Camera<T>>(), Lists(), tracer, 1, out.data()); }, "DRT_HIP_MAX_VIEWS"));
    CHECK(throws_with([&] { hip::render_pixels(scene, std::vector<Camera<T>>(65, cams[0]), Lists(65, {0u}), tracer, 1, out.data()); }, "DRT_HIP_MAX_VIEWS"));
    CHECK(throws_with([&] { hip::render_pixels(scene, cams, Lists{{0u}, {1u}}, tracer, 1, out.data()); }, "a pixel list per camera"));
    {
        std::vector<Camera<T>> other = cams;
        other[2] = Camera<T>(5, 3);
        CHECK(throws_with([&] { hip::render_pixels(scene, other, lists, tracer, 1, out.data()); }, "width or height"));
    }
    CHECK(throws_with([&] { hip::render_pixels(scene, cams, lists, tracer, 1, out.data(), hip::Options(), (const Vec3*)nullptr, std::vector<uint32_t>{1u, 2u}); }, "a seed per camera"));
    CHECK(throws_with([&] { hip::render_pixels(scene, cams, Lists{{}, {}, {}}, tracer, 1, out.data()); }, "an empty batch"));
    CHECK(throws_with([&] { hip::render_pixels(scene, cams, Lists{{0u}, {12u}, {}}, tracer, 1, out.data()); }, "outside the frame"));
    {
        hip::Options opt;
        opt.backward = opt.unbiased = true;
        CHECK(throws_with([&] { hip::render_pixels(scene, cams, lists, tracer, 1, out.data(), opt); }, "biased operator"));
        hip::Options l2;
        l2.sample_loss_l2 = true;
        CHECK(throws_with([&] { hip::render_pixels(scene, cams, lists, tracer, 1, out.data(), l2); }, "biased operator"));
        hip::Options two;
        two.devices = {0, 1};
        CHECK(throws_with([&] { hip::render_pixels(scene, cams, lists, tracer, 1, out.data(), two); }, "one device"));
    }
    CHECK(throws_with([&] { hip::render_pixels(scene, cams, lists, tracer, 1, (Vec3*)nullptr); }, "nothing to compute"));
    std::printf("ok\n");
    return 0;
}

static int device_checks()
{
    const std::size_t W = 20, H = 14, spp = 3, NP = W * H;
    const uint32_t seed = 11;
    Pathtracer<T> tracer(1.0, 4);
    std::vector<Camera<T>> cams = three_cameras(W, H);
    // unsorted lists with repeats: 70 entries (more than a wave), none, 9
    Lists lists(3);
    for (uint32_t k = 0; k < 70; ++k)
        lists[0].push_back((k * 97u + 13u) % (uint32_t)NP);
    lists[0][40] = lists[0][3];
    for (uint32_t k = 0; k < 9; ++k)
        lists[2].push_back((k * 31u + 200u) % (uint32_t)NP);
    lists[2][8] = lists[2][0];
    const std::size_t E = lists[0].size() + lists[2].size();
    // adjoints of values a float holds exactly
    std::vector<Vec3> adj(E);
    for (std::size_t i = 0; i < E; ++i)
        adj[i] = Vec3{0.25 * double(i % 7) - 0.5, 0.125 * double(i % 5), 1.5 - 0.25 * double(i % 3)};
    hip::Options opt;
    opt.backward = true;
    opt.f64 = true;
    opt.seed = seed;

    Room a;
    Scene<T> sa = a.scene();
    std::vector<Vec3> got(E, Vec3(0.));
    const hip::Stats st = hip::render_pixels(sa, cams, lists, tracer, spp, got.data(), opt, adj.data());
    CHECK(st.paths == E * spp);

    // the host API's own loop (render.cpp:72-86) over the listed pixels on the device's per-path streams
    Room h;
    Scene<T> sh = h.scene();
    std::vector<Vec3> cpu(E, Vec3(0.));
    std::size_t e = 0;
    for (std::size_t v = 0; v < 3; ++v)
        for (uint32_t pixel : lists[v]) {
            const std::size_t x = pixel % W, y = pixel / W;
            for (std::size_t i = 0; i < spp; ++i) {
                random::begin_path(seed, (uint64_t)pixel * spp + i);
                Vec3 dir;
                double pdf;
                std::tie(dir, pdf) = cams[v].sample(x, y);
                Var3 radiance = tracer.trace(sh, cams[v].eye(), dir);
                cpu[e] += radiance.detach() / pdf / double(spp);
                if (radiance.requires_grad())
                    radiance.backward(adj[e]);
            }
            ++e;
        }
    random::use_libc();
    double g_worst = 0, g_scale = 0, i_worst = 0, i_scale = 0;
    for (std::size_t p = 0; p < 4; ++p)
        for (int c = 0; c < 3; ++c) {
            g_scale = std::fmax(g_scale, std::fabs(h.params()[p]->grad()[c]));
            g_worst = std::fmax(g_worst, std::fabs(a.params()[p]->grad()[c] - h.params()[p]->grad()[c]));
        }
    for (std::size_t i = 0; i < E; ++i)
        for (int c = 0; c < 3; ++c) {
            i_scale = std::fmax(i_scale, std::fabs(cpu[i][c]));
            i_worst = std::fmax(i_worst, std::fabs(got[i][c] - cpu[i][c]));
        }
    hip::release_contexts();
    std::printf("against the host loop: gradient %.3g of %.3g, radiance %.3g of %.3g\n", g_worst, g_scale, i_worst, i_scale);
    // (the radiance is the f64 mean stored as float: half an ulp of the largest value on top of the bound)
    if (!(g_scale > 0 && g_worst <= 1e-9 * g_scale) || !(i_scale > 0 && i_worst <= (1e-9 + 6e-8) * i_scale)) {
        std::printf("FAILED\n");
        return 1;
    }
    std::printf("ok %.3g\n", g_worst / g_scale);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "device")
        return device_checks();
    return flatten_checks();
}
