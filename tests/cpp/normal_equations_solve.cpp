// NormalEquations::solve (include/drt/hip.hpp) on a fixed 3 x 4 x 4 system, no device: reads A (48 doubles), b (12), the requires_grad
// flags (4) and lambda from stdin, prints the 12 steps (step[p * 3 + ch]) -- tests/test_normal_equations_host_api.py compares with numpy.
#include <cstdio>
#include <drt/hip.hpp>

int main()
{
    drt::hip::NormalEquations<double> ne;
    ne.n_params = 4;
    ne.A.resize(48);
    ne.b.resize(12);
    ne.loss.assign(3, 0.0);
    ne.requires_grad.resize(4);
    for (double& v : ne.A)
        if (scanf("%lf", &v) != 1) return 2;
    for (double& v : ne.b)
        if (scanf("%lf", &v) != 1) return 2;
    for (uint8_t& f : ne.requires_grad) {
        int i;
        if (scanf("%d", &i) != 1) return 2;
        f = (uint8_t)i;
    }
    double lambda;
    if (scanf("%lf", &lambda) != 1) return 2;
    try {
        for (double s : ne.solve(lambda))
            printf("%.17g\n", s);
    } catch (const std::exception& e) {
        printf("threw: %s\n", e.what());
        return 1;
    }
    return 0;
}
