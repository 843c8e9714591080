// step_kernels.h -- the bookkeeping kernels of a training step (train_ops.hip): the step guard and its body (also run as
// a rider of the loss combine, loss_kernels.h), the view selection in front of a captured step, flat Adam over a plan
// of 1024-element blocks (one launch for every parameter segment, with the guard, the schedule and zero_grad folded in),
// and the two densification statistics kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "node_mlp.h"

namespace {

// Guard of a training step (dgs_step_guard; one thread).  status: [0] skip flag of this step, [1] number of skipped steps so far,
// [2] guarded steps so far.  skip[0] != 0 means "this step must not change anything" (see step_guard_kernel below).
__device__ __forceinline__ void step_guard_body(const int* skip, float* step_count, float* status, float* host_ring, int ring_len, float loss)
{
    const bool sk = skip && skip[0] != 0;
    if (!sk) step_count[0] += 1.0f;
    const float n_skipped = status[1] + (sk ? 1.0f : 0.0f);
    const float n_steps = status[2] + 1.0f;
    status[0] = sk ? 1.0f : 0.0f;
    status[1] = n_skipped;
    status[2] = n_steps;
    if (host_ring) {   // pinned host memory: (step index, skip flag, skipped so far, loss) of the last ring_len steps
        float* e = host_ring + 4 * ((long long)n_steps % ring_len);
        e[1] = sk ? 1.0f : 0.0f;
        e[2] = n_skipped;
        e[3] = loss;   // the step's loss: the host can read a history without a copy kernel per step
        __threadfence_system();
        e[0] = n_steps;   // written last: a reader that sees the index sees the payload
    }
}

// Guard of a training step (dgs_step_guard): skip[0] != 0 means "this step must not change anything" -- a rank's rasterizer
// ran out of list capacity and rendered background (under data parallelism the flag rides in the MAX all-reduce of the radii,
// so every rank sees the same value) -- and the update kernels return without touching parameters, moments, statistics or
// the step count.
__global__ void step_guard_kernel(const int* __restrict__ skip, float* __restrict__ step_count, float* __restrict__ status,
                                  float* __restrict__ host_ring, int ring_len, const float* __restrict__ loss)
{
    step_guard_body(skip, step_count, status, host_ring, ring_len, loss ? loss[0] : 0.0f);   // one thread
}

// First node of a captured step: the view of this replay.  row_out <- table[v] with v = override[0] if it is >= 0 (then reset to -1),
// else (counter[0] * stride + offset) mod nrows; counter[0] += 1.  A step that walks its views in the default order needs no host
// copy in front of the replay (the 256-byte row copy + the idle device behind it were ~10 us of every 0.8 ms step).
__global__ void __launch_bounds__(64) select_row_kernel(mlp::SelectArgs q) { mlp::select_row_body(q); }

// ---- flat Adam --------------------------------------------------------------------------------------------------
constexpr int kAdamSeg = 64;
constexpr int kAdamChunk = 1024;   // elements per workgroup (256 threads x 4: every load of a thread in flight at once -- with 16 the
                                   // update of the 0.5 M deformation parameters was four dependent memory round trips, 19 us)

struct AdamSegs {
    float* p[kAdamSeg];
    long long off[kAdamSeg + 1];
    float lr[kAdamSeg];
    // optional periodic learning-rate pattern inside a segment: element i uses lr2 when (i % period) >= split
    // (e.g. SH coefficients stored [P,16,3]: the DC term and the higher bands have different rates); period 0 = off
    float lr2[kAdamSeg];
    int period[kAdamSeg];
    int split[kAdamSeg];
    // optional exponential schedule of lr (get_expon_lr_func, utils/general_utils.py:49-83, lr_delay_steps = 0), evaluated on
    // the device from the step counter so that a captured step needs no host update: sched_steps 0 = constant
    float lr_final[kAdamSeg];
    float sched_steps[kAdamSeg];
    float sched_t0;
    // step origin of a segment: its bias corrections use t - t_origin.  torch.optim.Adam counts steps PER PARAMETER and skips
    // parameters without a gradient, so a parameter that joins the optimisation late (the reference's deformation and `feature`
    // after the warm-up, train_gui.py:281-285) starts at step 1 while the run's counter t is in the thousands
    float t_origin[kAdamSeg];
    float gscale;   // gradients are read as grad * gscale (data parallel: the bucket holds the SUM over ranks, gscale = 1 / world)
    int zero_grad;  // the gradient is cleared behind the read (optimizer.step() + zero_grad() in one pass; also on a skipped step)
};

// grad2 (nullable): a second gradient buffer of the same layout, ADDED to the first on the fly -- the two views of a step that were
// rendered concurrently keep a bucket each (Trainer.concurrent_views) and the update reads their sum without an adding pass.
// NT (DGS_ADAM_NT: 0 off, 1 moments + gradient = the default, 2 the parameter store too): the update's streams carry the non-temporal
// hint -- 320 MB per step that nothing reads again before the next step, passing through the L2s next to the working set of the node-MLP
// backward chain that runs beside the update (the step's critical path)
typedef float adam_f4 __attribute__((ext_vector_type(4)));
template <int NT>
__device__ __forceinline__ void adam_block(const AdamSegs& sg, const int2 pl, float* __restrict__ grad, float* __restrict__ m, float* __restrict__ v,
                                           const float t, float b1, float b2, float eps, const bool sk, const float* __restrict__ grad2)
{
    // pl = (segment, first element of this block inside the segment)
    const int s = pl.x;
    const long long seg_len = sg.off[s + 1] - sg.off[s];
    const float ts = fmaxf(t - sg.t_origin[s], 1.0f);
    const float bc1 = 1.0f - powf(b1, ts), bc2 = 1.0f - powf(b2, ts);
    float lr = sg.lr[s];
    if (sg.sched_steps[s] > 0.0f) {
        // the reference sets the rate AFTER optimizer.step(): step t runs at schedule(t - 1)
        const float tau = fminf(fmaxf((t - 1.0f + sg.sched_t0) / sg.sched_steps[s], 0.0f), 1.0f);
        lr = expf(logf(lr) * (1.0f - tau) + logf(sg.lr_final[s]) * tau);
    }
    const float step_size = lr / bc1, step_size2 = sg.lr2[s] / bc1, inv_sqrt_bc2 = 1.0f / sqrtf(bc2);
    const unsigned period = (unsigned)sg.period[s], split = (unsigned)sg.split[s];
    float* __restrict__ p = sg.p[s];
    const long long base = sg.off[s];
    auto update = [&](float g, float& mi, float& vi, float& pi, long long i) {
        mi = b1 * mi + (1.0f - b1) * g;
        vi = b2 * vi + (1.0f - b2) * g * g;
        const float ss = (period && (unsigned)(i % period) >= split) ? step_size2 : step_size;
        pi -= ss * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
    };
    static_assert(kAdamChunk == 4 * 256, "one 16-byte vector per thread and stream");
    const long long i0 = (long long)pl.y + 4 * threadIdx.x;
    // a thread owns 4 consecutive elements: one 16-byte access per stream instead of four 4-byte ones (which keep the address unit
    // busy four times as long: 28 accesses per 4 elements were ~40 us of it per launch) -- when the block's 4 KB of every stream
    // are 16-byte aligned and inside the segment
    const bool vec = ((base + pl.y) & 3) == 0 && (reinterpret_cast<size_t>(p + pl.y) & 15) == 0 && i0 + 3 < seg_len;
    if (vec) {
        float4* gq = reinterpret_cast<float4*>(grad + base + i0);
        float4* mq = reinterpret_cast<float4*>(m + base + i0);
        float4* vq = reinterpret_cast<float4*>(v + base + i0);
        float4* pq = reinterpret_cast<float4*>(p + i0);
        float4 g4;
        if (NT) { const adam_f4 t4 = __builtin_nontemporal_load(reinterpret_cast<const adam_f4*>(gq)); g4 = make_float4(t4.x, t4.y, t4.z, t4.w); }
        else g4 = *gq;
        if (grad2) {
            const float4 h4 = *reinterpret_cast<const float4*>(grad2 + base + i0);
            g4.x += h4.x; g4.y += h4.y; g4.z += h4.z; g4.w += h4.w;
        }
        if (sg.zero_grad) *gq = make_float4(0.f, 0.f, 0.f, 0.f);
        if (sk) return;
        float4 m4, v4, p4 = *pq;
        if (NT) {
            const adam_f4 a4 = __builtin_nontemporal_load(reinterpret_cast<const adam_f4*>(mq)), b4 = __builtin_nontemporal_load(reinterpret_cast<const adam_f4*>(vq));
            m4 = make_float4(a4.x, a4.y, a4.z, a4.w); v4 = make_float4(b4.x, b4.y, b4.z, b4.w);
        } else { m4 = *mq; v4 = *vq; }
        update(g4.x * sg.gscale, m4.x, v4.x, p4.x, i0);
        update(g4.y * sg.gscale, m4.y, v4.y, p4.y, i0 + 1);
        update(g4.z * sg.gscale, m4.z, v4.z, p4.z, i0 + 2);
        update(g4.w * sg.gscale, m4.w, v4.w, p4.w, i0 + 3);
        if (NT) {
            __builtin_nontemporal_store(adam_f4{m4.x, m4.y, m4.z, m4.w}, reinterpret_cast<adam_f4*>(mq));
            __builtin_nontemporal_store(adam_f4{v4.x, v4.y, v4.z, v4.w}, reinterpret_cast<adam_f4*>(vq));
            if (NT == 2) __builtin_nontemporal_store(adam_f4{p4.x, p4.y, p4.z, p4.w}, reinterpret_cast<adam_f4*>(pq));
            else *pq = p4;
        } else { *mq = m4; *vq = v4; *pq = p4; }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const long long i = i0 + k;
        if (i < seg_len) {
            const float g = (grad[base + i] + (grad2 ? grad2[base + i] : 0.0f)) * sg.gscale;
            if (sg.zero_grad) grad[base + i] = 0.0f;
            if (sk) continue;
            float mi = m[base + i], vi = v[base + i], pi = p[i];
            update(g, mi, vi, pi, i);
            m[base + i] = mi;
            v[base + i] = vi;
            p[i] = pi;
        }
    }
}

// nblocks plan entries over gridDim.x workgroups (at most 4096 by default: see the launch)
template <int NT>
__global__ void __launch_bounds__(256) adam_kernel(AdamSegs sg, const int2* __restrict__ plan, int nblocks, float* __restrict__ grad,
                                                   float* __restrict__ m, float* __restrict__ v, const float* __restrict__ step_count,
                                                   float b1, float b2, float eps, const int* __restrict__ skip, const float* __restrict__ grad2)
{
    const bool sk = skip && skip[0] != 0;   // guarded step (see step_guard_kernel)
    if (sk && !sg.zero_grad) return;
    const float t = step_count[0];
    for (int b = blockIdx.x; b < nblocks; b += gridDim.x) adam_block<NT>(sg, plan[b], grad, m, v, t, b1, b2, eps, sk, grad2);
}

long long adam_blocks(int nseg, const long long* off)
{
    long long nb = 0;
    for (int s = 0; s < nseg; s++) nb += (off[s + 1] - off[s] + kAdamChunk - 1) / kAdamChunk;
    return nb;
}

// ---- densification statistics (train_gui.py:411, gaussian_model.py:484-486) ----------------------------------------
// one view: visible = radii > 0; grad_norm = |dL/dmeans2D[:, :2]| where visible
__global__ void __launch_bounds__(256) densify_view_kernel(int P, const int* radii, const float* g_means2D, float* grad_norm,
                                                           float* visible, int* radii_vis)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int r = radii[i];
    const bool v = r > 0;
    const float gx = g_means2D[3 * i], gy = g_means2D[3 * i + 1];
    grad_norm[i] = v ? sqrtf(gx * gx + gy * gy) : 0.f;
    visible[i] = v ? 1.f : 0.f;
    radii_vis[i] = v ? r : 0;
}
// running statistics: xyz_gradient_accum += grad_norm, denom += visible, max_radii2D = max(max_radii2D, radii_vis)
__global__ void __launch_bounds__(256) densify_accum_kernel(int P, const float* grad_norm, const float* visible, const int* radii_vis,
                                                            float* accum, float* denom, int* max_radii, const int* skip)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P || (skip && skip[0] != 0)) return;
    accum[i] += grad_norm[i];
    denom[i] += visible[i];
    max_radii[i] = max(max_radii[i], radii_vis[i]);
}

}  // namespace
