// drt_loss.h -- the per-sample loss from the caller's own source (drt_hip_set_sample_loss / drt_hip_render_sample_loss).
//
// The reference's loop is `radiance = trace(...); loss = loss_func(radiance); loss.backward()` (README.md:93-98) with loss_func the
// caller's code.  Here that code is the body of
//     template <typename R> void sample_loss(const R* q, V3<R> L, V3<R> t, R& value, V3<R>& grad)
// which hiprtc compiles (drt_jit.h) from a generated header "drt_sample_loss.h", included under DRT_SAMPLE_LOSS: the library's own build
// knows no such function.  q[0 .. DRT_MAX_LOSS_VALUES) are the caller's constants: DATA, a kernel argument -- the source alone names the
// kernel in the compile cache.
//
// On the one-launch route (drt_path.h, its lines under DRT_SAMPLE_LOSS) the LOSS instantiation's two seeds call sample_loss where a path ends
// on a light, every lane adds the value of each sample it finishes into an fp64 sum of its own, and a wave writes ONE partial, its lanes
// added in a fixed order.
// On the tape route a path's radiance exists before its gradients are walked (k_radiance).  k_sample_seed, between k_radiance and the
// gradient walk, turns every path's radiance into its seed d value / d L IN PLACE and adds the path's value into its thread's fp64 sum;
// thread -> block in a fixed order, one partial per block and batch; k_loss_finish adds the partials of every batch of the shard -- either
// route's -- in a fixed order.  No atomics: the same call gives the same bits.
#pragma once

#include "drt_kernels.h"

struct LossValues {
    double q[DRT_MAX_LOSS_VALUES];
};

// a block's threads' sums into red[0], in a fixed order (all threads call)
__device__ inline void loss_block_sum(double (&red)[DRT_BLOCK], double v)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = DRT_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
}

#ifdef DRT_SAMPLE_LOSS
#include "drt_sample_loss.h"

// lacc[i]: in, the radiance of path i of the batch; out, its seed.  part[block]: the block's sum of the paths' values.
template <typename R>
__global__ void __launch_bounds__(DRT_BLOCK)
k_sample_seed(BatchArgs a, LossValues lv, const float* __restrict__ target, typename Q4<R>::T* __restrict__ lacc, double* __restrict__ part)
{
    typedef typename Q4<R>::T R4;
    __shared__ double red[DRT_BLOCK];
    R q[DRT_MAX_LOSS_VALUES];
#pragma unroll
    for (int k = 0; k < DRT_MAX_LOSS_VALUES; ++k)
        q[k] = (R)lv.q[k];
    double sum = 0.0;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n_paths; i += stride) {
        const uint32_t gp = global_pixel(a, a.p0 + i % a.Pb);
        const V3<R> t = mk<R>((R)target[(size_t)gp * 3], (R)target[(size_t)gp * 3 + 1], (R)target[(size_t)gp * 3 + 2]);
        const R4 l = lacc[i];
        R value = R(0);
        V3<R> grad = mk<R>(R(0), R(0), R(0));
        sample_loss<R>(q, mk<R>(l.x, l.y, l.z), t, value, grad);
        R4 o;
        o.x = grad.x; o.y = grad.y; o.z = grad.z; o.w = R(0);
        lacc[i] = o;
        sum += (double)value;
    }
    loss_block_sum(red, sum);
    if (threadIdx.x == 0)
        part[blockIdx.x] = red[0];
}
#endif

// out[0] = the sum of part[0 .. n): a strided sum per thread, then the block's tree, both in a fixed order (one block)
__global__ void __launch_bounds__(DRT_BLOCK)
k_loss_finish(const double* __restrict__ part, uint32_t n, double* __restrict__ out)
{
    __shared__ double red[DRT_BLOCK];
    double v = 0.0;
    for (uint32_t b = threadIdx.x; b < n; b += DRT_BLOCK)
        v += part[b];
    loss_block_sum(red, v);
    if (threadIdx.x == 0)
        out[0] = red[0];
}
