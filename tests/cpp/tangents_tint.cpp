// One tint over ten albedos through the host API: albedo_i = tint * base_i, one albedo per shape (the layout of cornell_shapes).
// The scene has ten device parameters beside the emission and three real degrees of freedom, d theta / d tint_ch = base_i[ch] on
// channel ch of every albedo.  drt::hip::normal_equations_along along those three directions (f64 mode) against the host API's own
// per-ray loop on Dual numbers, one Dual render per direction, on the device's per-path streams (tangent_dual.cpp):
//   A[ch][k][l] = sum_x T_k T_l,  b[ch][k] = sum_x T_k r,  loss[ch] = sum_x r^2   to 1e-9 of the sum of absolute terms,
//   the tangent images to 1e-9 of the largest value + the rounding of the float image the device returns.
// Prints "tangents_tint: ok" and exits 0, or reports what differs.
#include <cmath>
#include <cstdio>
#include <memory>
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

static const double BASE[10][3] = {{0.9, 0.8, 0.7}, {0.6, 0.9, 0.5}, {0.9, 0.2, 0.2}, {0.2, 0.9, 0.3}, {0.8, 0.8, 0.9},
                                   {0.7, 0.6, 0.8}, {0.9, 0.9, 0.6}, {0.5, 0.7, 0.9}, {0.3, 0.5, 0.9}, {0.9, 0.4, 0.7}};
static const double TINT[3] = {0.7, 0.6, 0.8};

// the room on number type S; `dch` >= 0: the albedos carry the dual part d albedo_i / d tint_dch
template <typename S, typename MakeColour>
struct Room {
    std::vector<Vector<S, 3, true>> albedo;
    Vector<S, 3, true> emission{Vector<S, 3>(S(1.)), true};
    std::vector<std::shared_ptr<BxDF<S>>> mat;
    std::shared_ptr<Emitter<S>> emitter = std::make_shared<AreaEmitter<S>>(emission);
    std::vector<std::unique_ptr<Shape<S>>> shapes;
    explicit Room(MakeColour colour)
    {
        typedef Vector<S, 3> V;
        for (int i = 0; i < 10; ++i) {
            albedo.emplace_back(colour(i), true);
            mat.push_back(std::make_shared<DiffuseBxDF<S>>(albedo.back()));
        }
        shapes.emplace_back(new Sphere<S>(V{0., 0., 3.}, 1., mat[0]));
        shapes.emplace_back(new Sphere<S>(V{-1., 1., 4.5}, 1., mat[1]));
        shapes.emplace_back(new Plane<S>(V{-1., 0., 0.}, -3., mat[2]));
        shapes.emplace_back(new Plane<S>(V{1., 0., 0.1}, -3., mat[3]));
        shapes.emplace_back(new Plane<S>(V{0., 0., -1.}, -6., mat[4]));
        shapes.emplace_back(new Plane<S>(V{0., 0., 1.}, 0., mat[5]));
        shapes.emplace_back(new Plane<S>(V{0., 1., 0.}, -3., mat[6]));
        shapes.emplace_back(new Plane<S>(V{0., -1., 0.}, -3., mat[7]));
        shapes.emplace_back(new Sphere<S>(V{1.5, -2., 4.}, 0.8, mat[8]));
        shapes.emplace_back(new Sphere<S>(V{-1.8, -2.2, 2.5}, 0.6, mat[9]));
        shapes.emplace_back(new Sphere<S>(V{0., 3., 3.}, 1., nullptr, emitter));
    }
    Scene<S> scene()
    {
        Scene<S> s;
        for (auto& p : shapes)
            s.push_back(p.get());
        return s;
    }
};

int main()
{
    const std::size_t W = 24, H = 18, spp = 4, npix = W * H;
    const uint32_t seed = 11;
    int bad = 0;
    struct Case { double absorb; std::size_t min_bounces; } cases[2] = {{1.0, 5}, {0.5, 1}};
    for (const Case& cs : cases) {
        // the host's own Dual loop, one render per direction
        std::vector<double> T(3 * npix * 3, 0.0);
        for (int k = 0; k < 3; ++k) {
            auto colour = [k](int i) {
                Vector<D, 3> c;
                for (int ch = 0; ch < 3; ++ch)
                    c[ch] = D(TINT[ch] * BASE[i][ch], ch == k ? BASE[i][ch] : 0.);
                return c;
            };
            Room<D, decltype(colour)> room(colour);
            Scene<D> scene = room.scene();
            Camera<D> cam(W, H);
            cam.look_at(Vector<D, 3>{0, 0, 0}, Vector<D, 3>{0, 0, 1});
            Pathtracer<D> tracer(cs.absorb, cs.min_bounces);
            for (std::size_t y = 0; y < H; ++y)
                for (std::size_t x = 0; x < W; ++x)
                    for (std::size_t i = 0; i < spp; ++i) {
                        random::begin_path(seed, (uint64_t)(y * W + x) * spp + i);
                        Vector<D, 3> dir;
                        double pdf;
                        std::tie(dir, pdf) = cam.sample(x, y);
                        auto radiance = tracer.trace(scene, cam.eye(), dir);
                        for (int c = 0; c < 3; ++c)
                            T[((std::size_t)k * npix + y * W + x) * 3 + c] += detach(radiance)[c].dual() / (pdf * double(spp));
                    }
            random::use_libc();
        }
        // the device: the same scene on doubles, the three directions as (handle, direction) pairs
        auto colour = [](int i) { return Vector<double, 3>{TINT[0] * BASE[i][0], TINT[1] * BASE[i][1], TINT[2] * BASE[i][2]}; };
        Room<double, decltype(colour)> room(colour);
        Scene<double> scene = room.scene();
        Camera<double> cam(W, H);
        cam.look_at(Vector<double, 3>{0, 0, 0}, Vector<double, 3>{0, 0, 1});
        Pathtracer<double> tracer(cs.absorb, cs.min_bounces);
        std::vector<hip::Direction<double>> dirs(3);
        for (int k = 0; k < 3; ++k)
            for (int i = 0; i < 10; ++i) {
                Vector<double, 3> d(0.);
                d[k] = BASE[i][k];
                dirs[k].push_back({room.albedo[i], d});
            }
        std::vector<Vector<double, 3>> residual(npix), img(npix), timg(3 * npix);
        for (std::size_t i = 0; i < npix; ++i)
            for (int c = 0; c < 3; ++c)
                residual[i][c] = double(float(std::sin(0.37 * double(i) + 1.3 * c)));      // (floats: what the ABI carries)
        hip::Options opt;
        opt.f64 = true;
        opt.seed = seed;
        const auto ne = hip::normal_equations_along(scene, cam, tracer, spp, dirs, opt, hip::TargetOrResidual<double>::residual(residual.data()),
                                                    img.data(), timg.data());
        double t_scale = 0, t_worst = 0;
        for (std::size_t i = 0; i < 3 * npix; ++i)
            for (int c = 0; c < 3; ++c) {
                t_scale = std::fmax(t_scale, std::fabs(T[i * 3 + c]));
                t_worst = std::fmax(t_worst, std::fabs(timg[i][c] - T[i * 3 + c]));
            }
        double s_worst = 0;
        for (int ch = 0; ch < 3; ++ch) {
            double loss = 0;
            for (std::size_t x = 0; x < npix; ++x)
                loss += residual[x][ch] * residual[x][ch];
            s_worst = std::fmax(s_worst, std::fabs(ne.loss[ch] - loss) / loss);
            for (int k = 0; k < 3; ++k) {
                double b = 0, babs = 0;
                for (std::size_t x = 0; x < npix; ++x) {
                    const double t = T[((std::size_t)k * npix + x) * 3 + ch] * residual[x][ch];
                    b += t;
                    babs += std::fabs(t);
                }
                if (babs > 0)
                    s_worst = std::fmax(s_worst, std::fabs(ne.b[ch * 3 + k] - b) / babs);
                else
                    bad += ne.b[ch * 3 + k] != 0.0;
                for (int l = 0; l < 3; ++l) {
                    double a = 0, aabs = 0;
                    for (std::size_t x = 0; x < npix; ++x) {
                        const double t = T[((std::size_t)k * npix + x) * 3 + ch] * T[((std::size_t)l * npix + x) * 3 + ch];
                        a += t;
                        aabs += std::fabs(t);
                    }
                    if (aabs > 0)
                        s_worst = std::fmax(s_worst, std::fabs(ne.A[(ch * 3 + k) * 3 + l] - a) / aabs);
                    else
                        bad += ne.A[(ch * 3 + k) * 3 + l] != 0.0;
                }
            }
        }
        std::printf("absorb %.1f from bounce %zu: tangent images %.3g of %.3g, sums %.3g of their absolute terms (%llu segments)\n",
                    cs.absorb, cs.min_bounces, t_worst, t_scale, s_worst, ne.stats.segments);
        if (!(t_scale > 0 && t_worst <= (1e-9 + std::ldexp(1.0, -24)) * t_scale && s_worst <= 1e-9))
            ++bad;
        // direction k moves channel k alone: solve() leaves the rows a channel does not depend on where they are and gives tint_ch the
        // damped step of its own 1 x 1 system
        const double lambda = 0.25;
        const std::vector<double> step = ne.solve(lambda);
        for (int ch = 0; ch < 3; ++ch)
            for (int k = 0; k < 3; ++k) {
                const double a = ne.A[(ch * 3 + k) * 3 + k];
                const double want = k == ch ? -ne.b[ch * 3 + k] / (a * (1.0 + lambda)) : 0.0;
                if (k == ch ? !(a > 0.0 && std::fabs(step[k * 3 + ch] - want) <= 1e-12 * std::fabs(want)) : (a != 0.0 || step[k * 3 + ch] != 0.0))
                    ++bad;
            }
    }
    hip::release_contexts();
    if (bad) {
        std::printf("FAILED (%d)\n", bad);
        return 1;
    }
    std::printf("tangents_tint: ok\n");
    return 0;
}
