// The unbiased losses of a frame under several parameter sets through the host API (drt::hip::render_param_sets_cross,
// drt_hip_render_param_sets_cross).
//   sets_cross refuse   no device: spp 1 (and 0), a missing target and every reverse-mode option throw
//   sets_cross device   the reference's scene (tangent_dual.cpp's Room), 24 x 18, spp 4 and 2, tracers (absorb 1.0, 5 bounces) and
//                       (0.5, 1), three parameter sets, a fixed target.  The host's own per-ray loop (one pass per set, on the device's
//                       per-path streams) keeps every sample's L_{k,s} and forms, BY DEFINITION -- the double loop over ordered pairs of
//                       samples, not the moment shortcut the device uses --
//                           loss~_k = sum_x 1 / (n (n - 1)) sum_{s != s'} (L_{k,s} - target) (L_{k,s'} - target)
//                           bias_k  = the same sum over ALL pairs / n^2 (the plain r_k^2), less the above
//                           the variance image = the pixel's share of bias_k, the image = the pixel's mean
//                       against the device in the f64 mode: sums to 1e-9 of the sum of the absolute per-pixel, per-pair terms, images to
//                       1e-9 of the largest value (the host's value rounded to the float the ABI carries), segment counts equal to a
//                       plain render of the same frame.
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

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

// the parameters of the reference's scene -- red, green, white, emission -- and three sets of them: set 0 the scene's own, the others with
// every channel moved (red's and green's zero channels too)
static const double VALUE[4][3] = {{0.5, 0., 0.}, {0., 0.5, 0.}, {0.5, 0.5, 0.5}, {1., 1., 1.}};
static const double SET[3][4][3] = {{{0.5, 0., 0.}, {0., 0.5, 0.}, {0.5, 0.5, 0.5}, {1., 1., 1.}},
                                    {{0.7, 0.1, 0.05}, {0.15, 0.35, 0.1}, {0.6, 0.45, 0.55}, {1.2, 0.9, 0.8}},
                                    {{0.3, 0.2, 0.25}, {0.05, 0.8, 0.3}, {0.35, 0.7, 0.4}, {0.7, 1.1, 1.3}}};

// the reference's scene (render.cpp:26-59; tangent_dual.cpp's Room), its parameters made by colour(p)
struct Room {
    typedef double S;
    typedef Vector<S, 3> V;
    Vector<S, 3, true> red, green, white, emission;
    std::shared_ptr<BxDF<S>> dred, dgreen, dwhite, spec;
    std::shared_ptr<Emitter<S>> emitter;
    Sphere<S> s1, s2;
    Plane<S> p1, p2, p3, p4, p5, p6;
    Sphere<S> light;
    template <typename F>
    explicit Room(F colour)
        : red(colour(0), true), green(colour(1), true), white(colour(2), true), emission(colour(3), true),
          dred(std::make_shared<DiffuseBxDF<S>>(red)), dgreen(std::make_shared<DiffuseBxDF<S>>(green)),
          dwhite(std::make_shared<DiffuseBxDF<S>>(white)), spec(std::make_shared<SpecularBxDF<S>>(white, 30)),
          emitter(std::make_shared<AreaEmitter<S>>(emission)),
          s1(V{0., 0., 3.}, 1., spec), s2(V{-1., 1., 4.5}, 1., dwhite),
          p1(V{-1., 0., 0.}, -3., dred), p2(V{1., 0., 0.1}, -3., dgreen), p3(V{0., 0., -1.}, -6., dwhite), p4(V{0, 0, 1}, 0, dwhite),
          p5(V{0., 1., 0.}, -3., dwhite), p6(V{0., -1., 0.}, -3., dwhite), light(V{0., 3., 3.}, 1., nullptr, emitter)
    {
    }
    Scene<S> scene() { return Scene<S>{&s1, &s2, &p1, &p2, &p3, &p4, &p5, &p6, &light}; }
};

static Vector<double, 3> plain_colour(int p) { return Vector<double, 3>{VALUE[p][0], VALUE[p][1], VALUE[p][2]}; }

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

static std::vector<hip::ParamSet<double>> sets_of(Room& room)
{
    Vector<double, 3, true>* handle[4] = {&room.red, &room.green, &room.white, &room.emission};
    std::vector<hip::ParamSet<double>> sets(3);
    for (int k = 0; k < 3; ++k)
        for (int p = 0; p < 4; ++p)
            sets[k].emplace_back(*handle[p], Vector<double, 3>{SET[k][p][0], SET[k][p][1], SET[k][p][2]});
    return sets;
}

static int refuse_checks()
{
    Room room(plain_colour);
    Scene<double> scene = room.scene();
    Camera<double> cam(4, 3);
    cam.look_at(Vector<double, 3>{0, 0, 0}, Vector<double, 3>{0, 0, 1});
    Pathtracer<double> tracer(1.0, 2);
    const std::vector<hip::ParamSet<double>> sets = sets_of(room);
    std::vector<Vector<double, 3>> target(12, Vector<double, 3>(0.25));
    CHECK(throws_with([&] { hip::render_param_sets_cross(scene, cam, tracer, 1, sets, target.data()); }, "spp < 2"));
    CHECK(throws_with([&] { hip::render_param_sets_cross(scene, cam, tracer, 0, sets, target.data()); }, "spp < 2"));
    CHECK(throws_with([&] { hip::render_param_sets_cross(scene, cam, tracer, 4, sets, (const Vector<double, 3>*)nullptr); }, "target"));
    hip::Options back, unb, l2;
    back.backward = true;
    unb.unbiased = true;
    l2.sample_loss_l2 = true;
    Vector<double, 3>* none = nullptr;
    for (const hip::Options* o : {&back, &unb, &l2})
        CHECK(throws_with([&] { hip::render_param_sets_cross(scene, cam, tracer, 4, sets, target.data(), none, none, *o); }, "reverse-mode"));
    std::printf("ok\n");
    return 0;
}

static int device_checks()
{
    const std::size_t W = 24, H = 18, npix = W * H;
    const int K = 3;
    const uint32_t seed = 11;
    int bad = 0;
    double worst_sum = 0, worst_img = 0;
    std::vector<Vector<double, 3>> target(npix);
    for (std::size_t i = 0; i < npix; ++i)
        for (int c = 0; c < 3; ++c)
            target[i][c] = double(float(0.3 + 0.2 * std::sin(0.37 * double(i) + 1.3 * c)));      // (floats: what the ABI carries)
    struct Case { double absorb; std::size_t min_bounces; std::size_t spp; } cases[4] = {{1.0, 5, 4}, {0.5, 1, 4}, {1.0, 5, 2}, {0.5, 1, 2}};
    for (const Case& cs : cases) {
        const std::size_t n = cs.spp;
        // the host's own loop, one pass per set: every sample's L_{k,s}
        std::vector<double> L((std::size_t)K * npix * n * 3, 0.0);
        for (int k = 0; k < K; ++k) {
            Room room([k](int p) { return Vector<double, 3>{SET[k][p][0], SET[k][p][1], SET[k][p][2]}; });
            Scene<double> scene = room.scene();
            Camera<double> cam(W, H);
            cam.look_at(Vector<double, 3>{0, 0, 0}, Vector<double, 3>{0, 0, 1});
            Pathtracer<double> tracer(cs.absorb, cs.min_bounces);
            for (std::size_t y = 0; y < H; ++y)
                for (std::size_t x = 0; x < W; ++x)
                    for (std::size_t i = 0; i < n; ++i) {
                        random::begin_path(seed, (uint64_t)(y * W + x) * n + i);
                        Vector<double, 3> dir;
                        double pdf;
                        std::tie(dir, pdf) = cam.sample(x, y);
                        auto radiance = tracer.trace(scene, cam.eye(), dir);
                        for (int c = 0; c < 3; ++c)
                            L[(((std::size_t)k * npix + y * W + x) * n + i) * 3 + c] = detach(radiance)[c] / pdf;
                    }
            random::use_libc();
        }
        // by definition: ordered pairs of samples
        const double pairs = double(n) * double(n - 1), all = double(n) * double(n);
        double loss[K][3] = {}, lossabs[K][3] = {}, bias[K][3] = {}, biasabs[K][3] = {};
        std::vector<double> mean((std::size_t)K * npix * 3), var((std::size_t)K * npix * 3);
        for (int k = 0; k < K; ++k)
            for (std::size_t x = 0; x < npix; ++x)
                for (int ch = 0; ch < 3; ++ch) {
                    const double tg = target[x][ch];
                    const double* Lk = &L[(((std::size_t)k * npix + x) * n) * 3 + ch];
                    double m = 0;
                    for (std::size_t s = 0; s < n; ++s)
                        m += Lk[s * 3];
                    mean[((std::size_t)k * npix + x) * 3 + ch] = m / double(n);
                    double cross = 0, crossabs = 0, plain = 0, plainabs = 0;
                    for (std::size_t s = 0; s < n; ++s)
                        for (std::size_t s2 = 0; s2 < n; ++s2) {
                            const double term = (Lk[s * 3] - tg) * (Lk[s2 * 3] - tg);
                            plain += term / all;
                            plainabs += std::fabs(term) / all;
                            if (s != s2) {
                                cross += term / pairs;
                                crossabs += std::fabs(term) / pairs;
                            }
                        }
                    loss[k][ch] += cross;
                    lossabs[k][ch] += crossabs;
                    bias[k][ch] += plain - cross;
                    biasabs[k][ch] += plainabs + crossabs;
                    var[((std::size_t)k * npix + x) * 3 + ch] = plain - cross;
                }
        // the device: the scene with its own parameters, the sets as (handle, value) pairs
        Room room(plain_colour);
        Scene<double> scene = room.scene();
        Camera<double> cam(W, H);
        cam.look_at(Vector<double, 3>{0, 0, 0}, Vector<double, 3>{0, 0, 1});
        Pathtracer<double> tracer(cs.absorb, cs.min_bounces);
        const std::vector<hip::ParamSet<double>> sets = sets_of(room);
        std::vector<Vector<double, 3>> imgs((std::size_t)K * npix), vimgs((std::size_t)K * npix), plain_img(npix);
        hip::Options opt;
        opt.f64 = true;
        opt.seed = seed;
        const auto sc = hip::render_param_sets_cross(scene, cam, tracer, n, sets, target.data(), imgs.data(), vimgs.data(), opt);
        const hip::Stats plain_stats = hip::render(scene, cam, tracer, n, plain_img.data(), opt);
        CHECK(sc.losses.size() == (std::size_t)K * 3 && sc.biases.size() == (std::size_t)K * 3);
        double s_worst = 0;
        auto sum_check = [&](double got, double want, double scale) {
            if (scale > 0)
                s_worst = std::fmax(s_worst, std::fabs(got - want) / scale);
            else
                bad += got != 0.0;
        };
        for (int k = 0; k < K; ++k)
            for (int ch = 0; ch < 3; ++ch) {
                sum_check(sc.losses[k * 3 + ch], loss[k][ch], lossabs[k][ch]);
                sum_check(sc.biases[k * 3 + ch], bias[k][ch], biasabs[k][ch]);
            }
        // images: the device's floats against the host's values rounded to float
        double i_worst = 0;
        auto image_check = [&](const std::vector<Vector<double, 3>>& got, const std::vector<double>& want) {
            double scale = 0, worst = 0;
            for (std::size_t i = 0; i < want.size(); ++i) {
                scale = std::fmax(scale, std::fabs(want[i]));
                worst = std::fmax(worst, std::fabs(got[i / 3][i % 3] - double(float(want[i]))));
            }
            if (!(scale > 0))
                ++bad;
            else
                i_worst = std::fmax(i_worst, worst / scale);
        };
        image_check(imgs, mean);
        image_check(vimgs, var);
        std::printf("absorb %.1f from bounce %zu, spp %zu: sums %.3g of their absolute terms, images %.3g of the largest value (%llu segments, "
                    "plain render %llu)\n", cs.absorb, cs.min_bounces, n, s_worst, i_worst, (unsigned long long)sc.stats.segments,
                    (unsigned long long)plain_stats.segments);
        if (!(s_worst <= 1e-9 && i_worst <= 1e-9 && sc.stats.segments == plain_stats.segments && sc.stats.segments > 0))
            ++bad;
        worst_sum = std::fmax(worst_sum, s_worst);
        worst_img = std::fmax(worst_img, i_worst);
    }
    hip::release_contexts();
    if (bad) {
        std::printf("FAILED (%d)\n", bad);
        return 1;
    }
    std::printf("ok %.3g %.3g\n", worst_sum, worst_img);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "device")
        return device_checks();
    return refuse_checks();
}
