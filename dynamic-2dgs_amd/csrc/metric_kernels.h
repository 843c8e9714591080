// metric_kernels.h -- image metrics of an evaluation run on gfx950 (train_ops.hip): for every plane of a batch [B,C,H,W] the three
// sums behind PSNR, SSIM and one level of MS-SSIM, and optionally the next level of the MS-SSIM pyramid, in ONE launch.
//   SE = sum (a - b)^2 over all H x W pixels, S = sum ssim, CS = sum cs over the output domain (include/dgs_train_ops.h)
// image_metrics_kernel is laid out like ssim_fwd_kernel (loss_kernels.h), whose tile, window and thread maps it shares: a 256-thread
// workgroup owns a 54 x 28 output tile of one plane, vertical pass straight from global memory (a lane per input column, clamped
// addresses, zeros selected afterwards), horizontal pass from LDS, window weights in VGPRs.  What differs:
//   * `shift`: the window's first tap relative to the output pixel.  5 = the zero-padded H x W domain ("same"), 0 = the
//     (H - 10) x (W - 10) domain without padding ("valid": the inputs of output (y, x) are rows y .. y + 10, columns x .. x + 10);
//   * the 8-bit round trip applied to both images as they are loaded (`quantize`);
//   * the squared error of the tile's OWN input pixels.  In valid mode the output tiles do not cover the last 10 rows and columns of
//     the input: the last tile of a row / column owns them (they are among the 64 columns / 38 rows it loads anyway);
//   * the contrast-structure term next to the full SSIM term, and no derivative maps;
//   * one slot of three floats per workgroup, nothing atomic: image_metrics_combine_kernel (one workgroup per plane, behind the
//     kernel boundary) adds a plane's slots in float64 in a fixed order, so a plane's result is the same bits in every run and in
//     every batch it is part of;
//   * the pooled planes (2 x 2 mean, stride 2, one row / column of zeros in front of an odd axis, divisor 4): a workgroup writes the
//     pooled pixels of its tile, re-reading their four taps (L1 / L2 hits: it has just loaded them); consecutive threads write
//     consecutive pixels of a pooled row, so the stores are whole row segments.
#pragma once
#include <hip/hip_runtime.h>

#include "loss_kernels.h"
#include "train_common.h"

namespace {

struct MetricArgs {
    int H, W;              // plane size
    int OH, OW;            // output domain of the SSIM maps
    int shift;             // kR: same, 0: valid
    int quantize;
    const float* pred; const float* gt;
    float* partial;        // [plane][tile][3] = SE, S, CS
    float* pooled_pred; float* pooled_gt; int PH, PW;   // next pyramid level (both NULL: not produced)
};

constexpr int kMetricThreads = 256;
constexpr int kMetricLds = 5 * kTH * kLds + 12;   // floats
static_assert(kTW % 2 == 0 && kTH % 2 == 0, "a tile's pooled pixels start at (y0 / 2, x0 / 2)");

// grid of image_metrics_kernel: one workgroup per output tile and plane
inline dim3 metric_grid(int planes, int OH, int OW) { return dim3((OW + kTW - 1) / kTW, (OH + kTH - 1) / kTH, planes); }

// floor(clamp(x, 0, 1) * 255 + 0.5) / 255 with every operation rounded on its own, as the PyTorch expression rounds (a fused
// multiply-add would round once); the comparisons keep a NaN
__device__ __forceinline__ float metric_quant(float x)
{
#pragma clang fp contract(off)
    const float c = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
    const float p = c * 255.f;
    const float q = floorf(p + 0.5f);
    return __fdiv_rn(q, 255.f);
}

__global__ void __launch_bounds__(kMetricThreads) image_metrics_kernel(MetricArgs A, Gauss g)
{
    __shared__ float lds[kMetricLds];
    float (*s_v)[kTH][kLds] = reinterpret_cast<float (*)[kTH][kLds]>(lds);
    float* s_red = lds + 5 * kTH * kLds;
    const int H = A.H, W = A.W, s = A.shift;
    const int tid = threadIdx.x, col = tid & 63, rg = tid >> 6;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const bool lastx = blockIdx.x == gridDim.x - 1, lasty = blockIdx.y == gridDim.y - 1;
    const size_t plane = (size_t)blockIdx.z * H * W;
    const GlobalF p1 = (GlobalF)(A.pred + plane), p2 = (GlobalF)(A.gt + plane);
    float w[11];
    gauss_to_vgprs(g, w);
    float se = 0.f;
    {
        const int x = x0 + col - s;
        const bool xin = x >= 0 && x < W;
        const unsigned xc = (unsigned)min(max(x, 0), W - 1);
        float a[kPV + 10], b[kPV + 10];
#pragma unroll
        for (int j = 0; j < kPV + 10; j++) {   // clamped addresses, zeros (the padding) selected afterwards
            const int y = y0 + rg * kPV + j - s;
            const unsigned o = (unsigned)min(max(y, 0), H - 1) * (unsigned)W + xc;
            const bool in = xin && y >= 0 && y < H;
            float av = p1[o], bv = p2[o];
            if (A.quantize) { av = metric_quant(av); bv = metric_quant(bv); }
            a[j] = in ? av : 0.f;
            b[j] = in ? bv : 0.f;
        }
        // the squared error of the tile's own pixels: columns [0, kTW) and this wave's rows [0, kPV) behind the shift; the last tile
        // of a row / column also takes what lies beyond (valid mode: up to 10 more; same mode: nothing, it is outside the image)
        const int cc = col - s;
        const bool ownc = xin && cc >= 0 && (cc < kTW || lastx);
        const bool tall = lasty && rg == 3;
#pragma unroll
        for (int j = 0; j < kPV + 10; j++) {
            const int jj = j - s, y = y0 + rg * kPV + jj;
            const float d = a[j] - b[j];
            if (ownc && jj >= 0 && (jj < kPV || tall) && y < H) se += d * d;
        }
        // two sweeps as in ssim_fwd_body: means and the cross term from a, b, a b; then the squares in place of a, b
        {
            float ab[kPV + 10];
#pragma unroll
            for (int j = 0; j < kPV + 10; j++) ab[j] = a[j] * b[j];
#pragma unroll
            for (int o = 0; o < kPV; o++) {
                float m1 = 0.f, m2 = 0.f, q12 = 0.f;
#pragma unroll
                for (int k = 0; k < 11; k++) { m1 += w[k] * a[o + k]; m2 += w[k] * b[o + k]; q12 += w[k] * ab[o + k]; }
                const int r = rg * kPV + o;
                s_v[0][r][col] = m1; s_v[1][r][col] = m2; s_v[4][r][col] = q12;
            }
        }
#pragma unroll
        for (int j = 0; j < kPV + 10; j++) { a[j] *= a[j]; b[j] *= b[j]; asm volatile("" : "+v"(a[j]), "+v"(b[j])); }
#pragma unroll
        for (int o = 0; o < kPV; o++) {
            float q11 = 0.f, q22 = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) { q11 += w[k] * a[o + k]; q22 += w[k] * b[o + k]; }
            const int r = rg * kPV + o;
            s_v[2][r][col] = q11; s_v[3][r][col] = q22;
        }
    }
    __syncthreads();
    float vs = 0.f, vc = 0.f;
    if (tid < kTH * (kTW / kPH)) {
        const int r = tid / (kTW / kPH), c0 = (tid - r * (kTW / kPH)) * kPH;
        float res[5][kPH];
#pragma unroll
        for (int q = 0; q < 5; q++) {
            float v[kPH + 10];
#pragma unroll
            for (int j = 0; j < kPH + 10; j++) v[j] = s_v[q][r][c0 + j];
#pragma unroll
            for (int o = 0; o < kPH; o++) {
                float t = 0.f;
#pragma unroll
                for (int k = 0; k < 11; k++) t += w[k] * v[o + k];
                res[q][o] = t;
            }
            // one quantity's 16 reads and 66 FMAs at a time (see ssim_fwd_body)
            asm volatile("" : "+v"(res[q][0]), "+v"(res[q][1]), "+v"(res[q][2]), "+v"(res[q][3]), "+v"(res[q][4]), "+v"(res[q][5]) :: "memory");
        }
        const int y = y0 + r;
#pragma unroll
        for (int o = 0; o < kPH; o++) {
            const int x = x0 + c0 + o;
            const float mu1 = res[0][o], mu2 = res[1][o], s11 = res[2][o], s22 = res[3][o], s12 = res[4][o];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float sg1 = s11 - mu1_sq, sg2 = s22 - mu2_sq, sg12 = s12 - mu12;
            const float cs = (2.f * sg12 + kC2) / (sg1 + sg2 + kC2);
            const float m = (2.f * mu12 + kC1) / (mu1_sq + mu2_sq + kC1) * cs;
            if (x < A.OW && y < A.OH) { vs += m; vc += cs; }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) { se += __shfl_xor(se, d, 64); vs += __shfl_xor(vs, d, 64); vc += __shfl_xor(vc, d, 64); }
    if ((tid & 63) == 0) { s_red[tid >> 6] = se; s_red[4 + (tid >> 6)] = vs; s_red[8 + (tid >> 6)] = vc; }
    __syncthreads();
    if (tid < 3) {
        const size_t slot = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        A.partial[3 * slot + tid] = (s_red[4 * tid] + s_red[4 * tid + 1]) + (s_red[4 * tid + 2] + s_red[4 * tid + 3]);
    }
    if (A.pooled_pred) {
        typedef float __attribute__((address_space(1)))* GlobalW;
        const size_t pplane = (size_t)blockIdx.z * A.PH * A.PW;
        const GlobalW d1 = (GlobalW)(A.pooled_pred + pplane), d2 = (GlobalW)(A.pooled_gt + pplane);
        const int ph = H & 1, pw = W & 1;           // rows / columns of zeros in front
        const int px0 = x0 >> 1, py0 = y0 >> 1;
        const int px1 = lastx ? A.PW : min(px0 + kTW / 2, A.PW), py1 = lasty ? A.PH : min(py0 + kTH / 2, A.PH);
        const int nw = px1 - px0, n = nw * (py1 - py0);
        for (int i = tid; i < n; i += kMetricThreads) {
            const int r = i / nw, c = i - r * nw;
            const int py = py0 + r, px = px0 + c;
            const int ya = 2 * py - ph, xa = 2 * px - pw;   // >= -1; ya + 1 <= H - 1 and xa + 1 <= W - 1 for every pooled pixel
            const unsigned r0 = (unsigned)max(ya, 0) * (unsigned)W, r1 = (unsigned)(ya + 1) * (unsigned)W;
            const unsigned c0 = (unsigned)max(xa, 0), c1 = (unsigned)(xa + 1);
            float u[4] = {p1[r0 + c0], p1[r0 + c1], p1[r1 + c0], p1[r1 + c1]};
            float v[4] = {p2[r0 + c0], p2[r0 + c1], p2[r1 + c0], p2[r1 + c1]};
            if (A.quantize) {
#pragma unroll
                for (int k = 0; k < 4; k++) { u[k] = metric_quant(u[k]); v[k] = metric_quant(v[k]); }
            }
            const bool top = ya >= 0, left = xa >= 0;
            u[0] = top && left ? u[0] : 0.f; u[1] = top ? u[1] : 0.f; u[2] = left ? u[2] : 0.f;
            v[0] = top && left ? v[0] : 0.f; v[1] = top ? v[1] : 0.f; v[2] = left ? v[2] : 0.f;
            const unsigned oo = (unsigned)py * (unsigned)A.PW + (unsigned)px;
            d1[oo] = (((u[0] + u[1]) + u[2]) + u[3]) * 0.25f;
            d2[oo] = (((v[0] + v[1]) + v[2]) + v[3]) * 0.25f;
        }
    }
}

// out[plane][3] = the plane's slots added in float64: thread t takes slots t, t + 256, ... in order, then a fixed tree
__global__ void __launch_bounds__(kMetricThreads) image_metrics_combine_kernel(const float* __restrict__ partial, int ntiles, double* __restrict__ out)
{
    __shared__ double s_sum[3][kMetricThreads];
    const int tid = threadIdx.x;
    const float* p = partial + (size_t)blockIdx.x * ntiles * 3;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int i = tid; i < ntiles; i += kMetricThreads) { a0 += (double)p[3 * i]; a1 += (double)p[3 * i + 1]; a2 += (double)p[3 * i + 2]; }
    s_sum[0][tid] = a0; s_sum[1][tid] = a1; s_sum[2][tid] = a2;
    __syncthreads();
    for (int d = kMetricThreads / 2; d >= 1; d >>= 1) {
        if (tid < d) { s_sum[0][tid] += s_sum[0][tid + d]; s_sum[1][tid] += s_sum[1][tid + d]; s_sum[2][tid] += s_sum[2][tid + d]; }
        __syncthreads();
    }
    if (tid < 3) out[(size_t)blockIdx.x * 3 + tid] = s_sum[tid][0];
}

}  // namespace
