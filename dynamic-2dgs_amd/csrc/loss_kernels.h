// loss_kernels.h -- the training loss on gfx950 (train_ops.hip).
//   photometric: SSIM (utils/loss_utils.py:45-76 of the reference: five 11x11 depthwise convolutions plus autograd) and the
//     mean-|.| term, one kernel per direction.  A 256-thread workgroup owns a 54 x 28 output tile; the window is separable,
//     vertical pass straight from global memory (a lane per input column, no staging), horizontal pass from LDS.  The
//     forward leaves one partial per workgroup; the backward's last workgroup can sum the partials into the loss value
//     (combine_partials) and run the step guard behind it.
//   regularisers (normal consistency + distortion): forward and backward kernels on 16 x 16 tiles, and the fused kernel
//     that produces value and gradient in one pass on 30 x 14 tiles.
//   loss_fwd_merged_kernel: photometric forward and fused regularisers as alternating workgroups of one grid.
// The ssim_grid / reg16_grid / reg_fused_grid functions are the only place a grid is derived from an image size: the
// partial-buffer sizes the library reports and the grids it launches both come from them.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "step_kernels.h"
#include "train_common.h"

namespace {

constexpr int kR = 5;             // window radius (11 taps)
constexpr int kTW = 54, kTH = 28; // output tile of a 256-thread workgroup
constexpr int kCols = kTW + 2 * kR;   // 64 input columns: one per lane
constexpr int kPV = 7;            // output rows per thread of the vertical pass (4 waves x 7 rows)
constexpr int kPH = 6;            // output columns per thread of the horizontal pass (28 rows x 9 groups = 252 threads)
constexpr int kLds = kCols + 1;
static_assert(kCols == 64 && kTH == 4 * kPV && kTW % kPH == 0 && kTH * (kTW / kPH) <= 256, "thread maps below");

// grid of both SSIM kernels: one workgroup per tile and channel
inline dim3 ssim_grid(int C, int H, int W) { return dim3((W + kTW - 1) / kTW, (H + kTH - 1) / kTH, C); }

struct Gauss { float w[11]; };

Gauss make_gauss()
{
    // loss_utils.py:33-35: exp(-(x - 5)^2 / (2 * 1.5^2)) normalised, evaluated in float like the reference
    Gauss g;
    float s = 0.f;
    for (int i = 0; i < 11; i++) { g.w[i] = (float)std::exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); s += g.w[i]; }
    for (int i = 0; i < 11; i++) g.w[i] /= s;
    return g;
}
const Gauss& gauss() { static const Gauss g = make_gauss(); return g; }   // built on first use

constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

struct CombineArgs {
    const float* photo; int nphoto; const float* reg; int nreg; float inv_n; float lambda_dssim; float* out;
    // optional second rider: the step guard, run by the same thread right behind the loss it reports (g_step_count != nullptr)
    const int* g_skip; float* g_step_count; float* g_status; float* g_ring; int g_ring_len;
};

// loss = (1 - lambda) * sum(l1 partials) / n + lambda * (1 - sum(ssim partials) / n) + sum(regulariser partials)
// photo = [ssim partial per workgroup (nphoto) | l1 partial per workgroup (nphoto)], reg = [nreg]; one 256-thread workgroup
__device__ __forceinline__ void combine_partials(const CombineArgs& c, float (&s_red)[3][4])
{
    float a = 0.f, b = 0.f, r = 0.f;
    {
        float a4[4] = {0, 0, 0, 0}, b4[4] = {0, 0, 0, 0}, c4[4] = {0, 0, 0, 0};
        for (int i = threadIdx.x; i < c.nphoto; i += 1024)
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int k = i + 256 * u;
                a4[u] += k < c.nphoto ? c.photo[k] : 0.f;
                b4[u] += k < c.nphoto ? c.photo[c.nphoto + k] : 0.f;
            }
        for (int i = threadIdx.x; i < c.nreg; i += 1024)
#pragma unroll
            for (int u = 0; u < 4; u++) c4[u] += i + 256 * u < c.nreg ? c.reg[i + 256 * u] : 0.f;
        a = (a4[0] + a4[1]) + (a4[2] + a4[3]); b = (b4[0] + b4[1]) + (b4[2] + b4[3]); r = (c4[0] + c4[1]) + (c4[2] + c4[3]);
    }
    for (int d = 32; d >= 1; d >>= 1) { a += __shfl_xor(a, d, 64); b += __shfl_xor(b, d, 64); r += __shfl_xor(r, d, 64); }
    if ((threadIdx.x & 63) == 0) { s_red[0][threadIdx.x >> 6] = a; s_red[1][threadIdx.x >> 6] = b; s_red[2][threadIdx.x >> 6] = r; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
        b = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
        r = s_red[2][0] + s_red[2][1] + s_red[2][2] + s_red[2][3];
        const float loss = (1.0f - c.lambda_dssim) * b * c.inv_n + c.lambda_dssim * (1.0f - a * c.inv_n) + r;
        c.out[0] = loss;
        if (c.g_step_count) step_guard_body(c.g_skip, c.g_step_count, c.g_status, c.g_ring, c.g_ring_len, loss);
    }
}

__global__ void __launch_bounds__(256) loss_combine_kernel(CombineArgs c)
{
    __shared__ float s_red[3][4];
    combine_partials(c, s_red);
}

// Both SSIM kernels: separable 11-tap window over one 54 x 28 output tile per 256-thread workgroup.
//   pass 1, vertical, straight from global memory: a wave owns 7 output rows, a lane one of the tile's 64 input columns, and loads
//     its 17 input rows with fully coalesced 256-byte wave loads that are all in flight at once -- no staging of the inputs in LDS,
//     no staging barrier (the round-2 kernels staged a 42 x 42 window element by element: 14 dependent memory round trips per
//     workgroup, 39 us for the forward at 800 x 800 x 3; batching those loads gave 27 us, this layout 21: the two passes alone
//     are 11 us, writing the 23 MB of derivative maps the rest);
//   pass 2, horizontal, from LDS: thread = (row, 6 adjacent outputs), 16 reads per quantity.
// Every thread filters several adjacent outputs from one run of inputs held in registers (7 + 10 rows, 6 + 10 columns).  The
// window weights are copied into VGPRs: a VALU instruction with an SGPR source issues at 4.4 instead of 2.5 cycles on gfx950
// (profiles/r03_valu_issue_gfx950.txt).  LDS 36 KB forward / 22 KB backward.
__device__ __forceinline__ void gauss_to_vgprs(const Gauss& g, float (&w)[11])
{
#pragma unroll
    for (int k = 0; k < 11; k++) { w[k] = g.w[k]; asm volatile("" : "+v"(w[k])); }
}

struct SsimFwdArgs {
    int H, W;
    const float* img1; const float* img2;
    float* ssim_sum; float* dm_dmu1; float* dm_ds11; float* dm_ds12; float* l1_sum; float* partial;
    const float* const* img2_slot;
};
constexpr int kSsimFwdLds = 5 * kTH * kLds + 8;   // floats

// workgroup (bx, by, bz) of a (gx, gy, gz) grid; `lds` = kSsimFwdLds floats
__device__ __forceinline__ void ssim_fwd_body(const SsimFwdArgs& A, const Gauss& g, int bx, int by, int bz, int gx, int gy, int gz,
                                              float* __restrict__ lds)
{
    const int H = A.H, W = A.W;
    const float* __restrict__ img1 = A.img1;
    const float* __restrict__ img2 = A.img2_slot ? *A.img2_slot : A.img2;   // indirection: the comparison image is chosen per graph replay by rewriting one pointer
    float* __restrict__ dm_dmu1 = A.dm_dmu1; float* __restrict__ dm_ds11 = A.dm_ds11; float* __restrict__ dm_ds12 = A.dm_ds12;
    float (*s_v)[kTH][kLds] = reinterpret_cast<float (*)[kTH][kLds]>(lds);
    float* s_red = lds + 5 * kTH * kLds;
    const int tid = threadIdx.x, col = tid & 63, rg = tid >> 6;
    const int x0 = bx * kTW, y0 = by * kTH;
    const size_t plane = (size_t)bz * H * W;
    float w[11];
    gauss_to_vgprs(g, w);
    float l1 = 0.f;
    {
        const GlobalF p1 = (GlobalF)(img1 + plane), p2 = (GlobalF)(img2 + plane);
        const int x = x0 + col - kR;
        const bool xin = x >= 0 && x < W;
        const unsigned xc = (unsigned)min(max(x, 0), W - 1);
        float a[kPV + 10], b[kPV + 10];
#pragma unroll
        for (int j = 0; j < kPV + 10; j++) {   // clamped addresses, zeros (the conv2d padding) selected afterwards
            const int y = y0 + rg * kPV + j - kR;
            const unsigned o = (unsigned)min(max(y, 0), H - 1) * (unsigned)W + xc;
            const bool in = xin && y >= 0 && y < H;
            const float av = p1[o], bv = p2[o];
            a[j] = in ? av : 0.f;
            b[j] = in ? bv : 0.f;
        }
        const bool mine = col >= kR && col < kR + kTW && xin;   // the tile's own pixels: the mean-|.| term
#pragma unroll
        for (int o = 0; o < kPV; o++)
            if (mine && y0 + rg * kPV + o < H) l1 += fabsf(a[o + kR] - b[o + kR]);
        // two sweeps keep the live set near 100 registers (4 workgroups per CU): means and the cross term from a, b, a b; then the
        // squares in place of a, b
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
    float val = 0.f;
    float res[5][kPH];
    if (tid < kTH * (kTW / kPH)) {
        const int r = tid / (kTW / kPH), c0 = (tid - r * (kTW / kPH)) * kPH;
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
            // one quantity's 16 reads and 66 FMAs at a time (the compiler hoists all 80 reads otherwise, and spills)
            asm volatile("" : "+v"(res[q][0]), "+v"(res[q][1]), "+v"(res[q][2]), "+v"(res[q][3]), "+v"(res[q][4]), "+v"(res[q][5]) :: "memory");
        }
        const int y = y0 + r;
#pragma unroll
        for (int o = 0; o < kPH; o++) {
            const int x = x0 + c0 + o;
            const float mu1 = res[0][o], mu2 = res[1][o], s11 = res[2][o], s22 = res[3][o], s12 = res[4][o];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float sg1 = s11 - mu1_sq, sg2 = s22 - mu2_sq, sg12 = s12 - mu12;
            const float A = 2.f * mu12 + kC1, B = 2.f * sg12 + kC2, Cc = mu1_sq + mu2_sq + kC1, D = sg1 + sg2 + kC2;
            const float inv_cd = 1.0f / (Cc * D);
            const float m = A * B * inv_cd;
            if (x < W && y < H) val += m;
            // map = A B / (Cc D) with sigma1^2 = s11 - mu1^2, sigma12 = s12 - mu1 mu2 (loss_utils.py:59-71)
            res[0][o] = (2.f * mu2 * B - 2.f * mu2 * A) * inv_cd - m * (2.f * mu1 / Cc - 2.f * mu1 / D);
            res[1][o] = -m / D;
            res[2][o] = 2.f * A * inv_cd;
        }
    }
    if (dm_dmu1) {
        // The derivative maps leave through LDS: a thread's 6 adjacent outputs would be 4-byte stores 24 bytes apart (18 partial
        // cache lines per wave store; the three maps cost 12 of the kernel's 25 us that way), rows of 54 floats are 2-3 lines.
        __syncthreads();                       // every thread is done reading s_v
        if (tid < kTH * (kTW / kPH)) {
            const int r = tid / (kTW / kPH), c0 = (tid - r * (kTW / kPH)) * kPH;
#pragma unroll
            for (int o = 0; o < kPH; o++) { s_v[0][r][c0 + o] = res[0][o]; s_v[1][r][c0 + o] = res[1][o]; s_v[2][r][c0 + o] = res[2][o]; }
        }
        __syncthreads();
        typedef float __attribute__((address_space(1)))* GlobalW;
        const GlobalW d0 = (GlobalW)(dm_dmu1 + plane), d1 = (GlobalW)(dm_ds11 + plane), d2 = (GlobalW)(dm_ds12 + plane);
#pragma unroll
        for (int t = 0; t < (kTH * kTW + 255) / 256; t++) {
            const int i = tid + 256 * t, r = i / kTW, c = i - r * kTW;
            const int y = y0 + r, x = x0 + c;
            if (i < kTH * kTW && x < W && y < H) {
                const unsigned oo = (unsigned)y * (unsigned)W + (unsigned)x;
                d0[oo] = s_v[0][r][c]; d1[oo] = s_v[1][r][c]; d2[oo] = s_v[2][r][c];
            }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) { val += __shfl_xor(val, d, 64); l1 += __shfl_xor(l1, d, 64); }
    if ((tid & 63) == 0) { s_red[tid >> 6] = val; s_red[4 + (tid >> 6)] = l1; }
    __syncthreads();
    if (tid == 0) {
        const float vs = s_red[0] + s_red[1] + s_red[2] + s_red[3], vl = s_red[4] + s_red[5] + s_red[6] + s_red[7];
        if (A.partial) {
            // one slot per workgroup, summed by loss_combine_kernel: thousands of atomics on ONE address serialise in a
            // single L2 channel (~13 ns each) and were most of this kernel's run time
            const int nb = gx * gy * gz;
            const int b = (bz * gy + by) * gx + bx;
            A.partial[b] = vs;
            A.partial[nb + b] = vl;
        } else {
            atomicAdd(A.ssim_sum, vs);
            if (A.l1_sum) atomicAdd(A.l1_sum, vl);
        }
    }
}

__global__ void __launch_bounds__(256) ssim_fwd_kernel(SsimFwdArgs A, Gauss g)
{
    __shared__ float lds[kSsimFwdLds];
    ssim_fwd_body(A, g, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, gridDim.y, gridDim.z, lds);
}

__global__ void __launch_bounds__(256) ssim_bwd_kernel(int H, int W, float inv_n, float l1_coef, const float* __restrict__ img1,
                                                       const float* __restrict__ img2, Gauss g, const float* __restrict__ dm_dmu1,
                                                       const float* __restrict__ dm_ds11, const float* __restrict__ dm_ds12,
                                                       const float* __restrict__ dL_dmean, float* __restrict__ dL_dimg1,
                                                       const float* const* __restrict__ img2_slot, CombineArgs comb)
{
    if (img2_slot) img2 = *img2_slot;
    __shared__ float s_v[3][kTH][kLds];
    const int tid = threadIdx.x, col = tid & 63, rg = tid >> 6;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const size_t plane = (size_t)blockIdx.z * H * W;
    float w[11];
    gauss_to_vgprs(g, w);
    {
        const GlobalF p0 = (GlobalF)(dm_dmu1 + plane), p1 = (GlobalF)(dm_ds11 + plane), p2 = (GlobalF)(dm_ds12 + plane);
        const int x = x0 + col - kR;
        const bool xin = x >= 0 && x < W;
        const unsigned xc = (unsigned)min(max(x, 0), W - 1);
        float v0[kPV + 10], v1[kPV + 10], v2[kPV + 10];
#pragma unroll
        for (int j = 0; j < kPV + 10; j++) {
            const int y = y0 + rg * kPV + j - kR;
            const unsigned o = (unsigned)min(max(y, 0), H - 1) * (unsigned)W + xc;
            const bool in = xin && y >= 0 && y < H;
            const float a = p0[o], b = p1[o], c = p2[o];
            v0[j] = in ? a : 0.f;
            v1[j] = in ? b : 0.f;
            v2[j] = in ? c : 0.f;
        }
#pragma unroll
        for (int o = 0; o < kPV; o++) {
            float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) { t0 += w[k] * v0[o + k]; t1 += w[k] * v1[o + k]; t2 += w[k] * v2[o + k]; }
            const int r = rg * kPV + o;
            s_v[0][r][col] = t0; s_v[1][r][col] = t1; s_v[2][r][col] = t2;
        }
    }
    __syncthreads();
    // the epilogue works on row-contiguous elements (coalesced image reads and gradient stores: see ssim_fwd_kernel); its image
    // reads go out before the LDS pass
    constexpr int kEp = (kTH * kTW + 255) / 256;
    const GlobalF q1 = (GlobalF)(img1 + plane), q2 = (GlobalF)(img2 + plane);
    float i1[kEp], i2[kEp];
#pragma unroll
    for (int t = 0; t < kEp; t++) {
        const int i = min(tid + 256 * t, kTH * kTW - 1), r = i / kTW, c = i - r * kTW;
        const unsigned oo = (unsigned)min(y0 + r, H - 1) * (unsigned)W + (unsigned)min(x0 + c, W - 1);
        i1[t] = q1[oo]; i2[t] = q2[oo];
    }
    float res[3][kPH];
    if (tid < kTH * (kTW / kPH)) {
        const int r = tid / (kTW / kPH), c0 = (tid - r * (kTW / kPH)) * kPH;
#pragma unroll
        for (int q = 0; q < 3; q++) {
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
            asm volatile("" : "+v"(res[q][0]), "+v"(res[q][1]), "+v"(res[q][2]), "+v"(res[q][3]), "+v"(res[q][4]), "+v"(res[q][5]) :: "memory");
        }
    }
    __syncthreads();                           // every thread is done reading s_v
    if (tid < kTH * (kTW / kPH)) {
        const int r = tid / (kTW / kPH), c0 = (tid - r * (kTW / kPH)) * kPH;
#pragma unroll
        for (int o = 0; o < kPH; o++) { s_v[0][r][c0 + o] = res[0][o]; s_v[1][r][c0 + o] = res[1][o]; s_v[2][r][c0 + o] = res[2][o]; }
    }
    __syncthreads();
    const float gm = dL_dmean[0];
    typedef float __attribute__((address_space(1)))* GlobalW;
    const GlobalW dst = (GlobalW)(dL_dimg1 + plane);
#pragma unroll
    for (int t = 0; t < kEp; t++) {
        const int i = tid + 256 * t, r = i / kTW, c = i - r * kTW;
        const int y = y0 + r, x = x0 + c;
        if (i < kTH * kTW && x < W && y < H) {
            // the zero-padded symmetric window is its own adjoint
            // inv_n scales the SSIM-map adjoint, l1_coef the sign(img1 - img2) of an optional mean-|.| term
            const float df = i1[t] - i2[t];
            const float sg = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
            dst[(unsigned)y * (unsigned)W + (unsigned)x] = ((s_v[0][r][c] + 2.f * i1[t] * s_v[1][r][c] + i2[t] * s_v[2][r][c]) * inv_n + l1_coef * sg) * gm;
        }
    }
    // optional rider: the LAST workgroup of the grid also sums the forward kernels' partials into the loss value (the train step
    // launches this kernel after both of them; a one-workgroup kernel of its own cost 5-8 us of the replayed step)
    if (comb.out && blockIdx.x == gridDim.x - 1 && blockIdx.y == gridDim.y - 1 && blockIdx.z == gridDim.z - 1) {
        __shared__ float s_red[3][4];
        combine_partials(comb, s_red);
    }
}

// ---- fused regulariser loss -----------------------------------------------------------------------------------------
__device__ __forceinline__ float clean_depth(float d)  // torch.nan_to_num(x, 0, 0): nan -> 0, +inf -> 0, -inf -> lowest
{
    if (d != d) return 0.f;
    if (d == INFINITY) return 0.f;
    if (d == -INFINITY) return -3.4028234663852886e38f;
    return d;
}

struct RegArgs {
    int H, W;
    const float* allmap; const float* rays_d; const float* rays_o; const float* wvt;
    float ln, ld;
    const float* const* rays_slot;   // non-null: rays_d = *rays_slot (chosen per graph replay by rewriting one pointer)
    int write_all;                   // backward: also store the zeros of planes 0, 1, 7 and of the border (caller zero-fills plane 5 only)
    float* zero_plane;               // forward: optional [H,W] plane to clear (the backward's atomics target: saves its fill launch)
};

// back-projected point of pixel (y, x)
__device__ __forceinline__ void reg_point(const RegArgs& a, int y, int x, float* p)
{
    const size_t q = (size_t)y * a.W + x;
    const float d = clean_depth(a.allmap[5 * (size_t)a.H * a.W + q]);
    p[0] = d * a.rays_d[3 * q] + a.rays_o[0];
    p[1] = d * a.rays_d[3 * q + 1] + a.rays_o[1];
    p[2] = d * a.rays_d[3 * q + 2] + a.rays_o[2];
}

// un-normalised normal v = dx x dy at an interior pixel, dx = p[y+1] - p[y-1], dy = p[x+1] - p[x-1]
__device__ __forceinline__ void reg_cross(const RegArgs& a, int y, int x, float* dx, float* dy, float* v)
{
    float pu[3], pd[3], pl[3], pr[3];
    reg_point(a, y + 1, x, pd); reg_point(a, y - 1, x, pu); reg_point(a, y, x + 1, pr); reg_point(a, y, x - 1, pl);
    for (int c = 0; c < 3; c++) { dx[c] = pd[c] - pu[c]; dy[c] = pr[c] - pl[c]; }
    v[0] = dx[1] * dy[2] - dx[2] * dy[1];
    v[1] = dx[2] * dy[0] - dx[0] * dy[2];
    v[2] = dx[0] * dy[1] - dx[1] * dy[0];
}

// grid of regloss_fwd_kernel / regloss_bwd_kernel: 16 x 16 pixels per workgroup
inline dim3 reg16_grid(int H, int W) { return dim3((W + 15) / 16, (H + 15) / 16); }

__global__ void __launch_bounds__(256) regloss_fwd_kernel(RegArgs a, float* loss, float* partial)
{
    if (a.rays_slot) a.rays_d = *a.rays_slot;
    __shared__ float s_red[4];
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    const size_t HW = (size_t)a.H * a.W;
    float val = 0.f;
    if (x < a.W && y < a.H) {
        const size_t q = (size_t)y * a.W + x;
        if (a.zero_plane) a.zero_plane[q] = 0.f;
        float dot = 0.f;
        if (x >= 1 && y >= 1 && x < a.W - 1 && y < a.H - 1) {
            float dx[3], dy[3], v[3];
            reg_cross(a, y, x, dx, dy, v);
            const float L = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            const float inv = a.allmap[HW + q] / fmaxf(L, 1e-12f);  // normalize(), then * alpha
            const float nv[3] = {a.allmap[2 * HW + q], a.allmap[3 * HW + q], a.allmap[4 * HW + q]};
            for (int c = 0; c < 3; c++) {
                const float nw = nv[0] * a.wvt[4 * c] + nv[1] * a.wvt[4 * c + 1] + nv[2] * a.wvt[4 * c + 2];  // n_view @ wvt[:3,:3].T
                dot += nw * v[c] * inv;
            }
        }
        val = (a.ln * (1.f - dot) + a.ld * a.allmap[6 * HW + q]) / (float)HW;
    }
    for (int d = 32; d >= 1; d >>= 1) val += __shfl_xor(val, d, 64);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = val;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float v = s_red[0] + s_red[1] + s_red[2] + s_red[3];
        if (partial) partial[blockIdx.y * gridDim.x + blockIdx.x] = v;   // see ssim_fwd_kernel
        else atomicAdd(loss, v);
    }
}

__global__ void __launch_bounds__(256) regloss_bwd_kernel(RegArgs a, const float* g, float* d_allmap)
{
    if (a.rays_slot) a.rays_d = *a.rays_slot;
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= a.W || y >= a.H) return;
    const size_t HW = (size_t)a.H * a.W, q = (size_t)y * a.W + x;
    const float gs = g[0] / (float)HW;
    d_allmap[6 * HW + q] = gs * a.ld;
    const bool interior = x >= 1 && y >= 1 && x < a.W - 1 && y < a.H - 1;
    if (a.write_all) {
        d_allmap[q] = 0.f; d_allmap[HW + q] = 0.f; d_allmap[7 * HW + q] = 0.f;
        if (!interior) { d_allmap[2 * HW + q] = 0.f; d_allmap[3 * HW + q] = 0.f; d_allmap[4 * HW + q] = 0.f; }
    }
    if (!interior) return;
    float dx[3], dy[3], v[3];
    reg_cross(a, y, x, dx, dy, v);
    const float L = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const float alpha = a.allmap[HW + q];
    const float denom = fmaxf(L, 1e-12f);
    const float n[3] = {v[0] / denom, v[1] / denom, v[2] / denom};
    const float nv[3] = {a.allmap[2 * HW + q], a.allmap[3 * HW + q], a.allmap[4 * HW + q]};
    float nw[3];
    for (int c = 0; c < 3; c++) nw[c] = nv[0] * a.wvt[4 * c] + nv[1] * a.wvt[4 * c + 1] + nv[2] * a.wvt[4 * c + 2];
    const float k = -gs * a.ln;
    // d / d rend_normal (view space): -lambda/HW * wvt[:3,:3]^T-rotated surf_normal
    for (int kk = 0; kk < 3; kk++) {
        float acc = 0.f;
        for (int c = 0; c < 3; c++) acc += a.wvt[4 * c + kk] * (n[c] * alpha);
        d_allmap[(2 + kk) * HW + q] = k * acc;
    }
    // d / d n (alpha is detached), then through F.normalize and the cross product
    float dn[3] = {k * nw[0] * alpha, k * nw[1] * alpha, k * nw[2] * alpha}, dv[3];
    if (L >= 1e-12f) {
        const float nd = n[0] * dn[0] + n[1] * dn[1] + n[2] * dn[2];
        for (int c = 0; c < 3; c++) dv[c] = (dn[c] - n[c] * nd) / L;
    } else {
        for (int c = 0; c < 3; c++) dv[c] = dn[c] / 1e-12f;
    }
    const float ddx[3] = {dy[1] * dv[2] - dy[2] * dv[1], dy[2] * dv[0] - dy[0] * dv[2], dy[0] * dv[1] - dy[1] * dv[0]};  // dy x dv
    const float ddy[3] = {dv[1] * dx[2] - dv[2] * dx[1], dv[2] * dx[0] - dv[0] * dx[2], dv[0] * dx[1] - dv[1] * dx[0]};  // dv x dx
    float* dd = d_allmap + 5 * HW;
    const int ys[4] = {y + 1, y - 1, y, y}, xs[4] = {x, x, x + 1, x - 1};
    const float sg[4] = {1.f, -1.f, 1.f, -1.f};
    for (int i = 0; i < 4; i++) {
        const size_t qq = (size_t)ys[i] * a.W + xs[i];
        const float raw = a.allmap[5 * HW + qq];
        if (raw != raw || raw == INFINITY || raw == -INFINITY) continue;  // nan_to_num has zero gradient there
        const float* gd = i < 2 ? ddx : ddy;
        atomicAdd(dd + qq, sg[i] * (gd[0] * a.rays_d[3 * qq] + gd[1] * a.rays_d[3 * qq + 1] + gd[2] * a.rays_d[3 * qq + 2]));
    }
}

// ---- regularisers, value AND gradient in one kernel (unit upstream gradient) -----------------------------------------
// The train step differentiates loss = photometric + regularisers with dL/dloss = 1, so the regularisers' gradient image depends on
// the rasterizer outputs only and can be produced next to the value: one pass over the allmap instead of two (regloss_fwd_kernel +
// regloss_bwd_kernel read the same planes twice), and the depth gradient is GATHERED -- every pixel sums the four neighbouring
// normals' contributions from LDS -- instead of 4 float atomics per pixel into a pre-cleared plane (2.6 M atomics at 800 x 800).
//   workgroup = 30 x 14 pixels; normals ("centres") are needed on 32 x 16, back-projected points on 34 x 18
//   phase 1: points of the 34 x 18 region -> LDS (every global load of the 3 trips in flight before the first LDS store)
//   phase 2: thread = centre (2 trips of 32 x 8): cross product, normalisation, loss term, d/d rend_normal, and the two
//            vectors ddx = dy x dv, ddy = dv x dx its four neighbours' points receive -> LDS
//   phase 3: the centre's own thread gathers  +ddx(y-1) - ddx(y+1) + ddy(x-1) - ddy(x+1),  dots with its ray, stores all 8 planes
// 11 + 23 -> 17 us at 800 x 800 (forward + backward kernels -> this one).
constexpr int kRW = 30, kRH = 14;                 // own pixels of a workgroup
constexpr int kCW = kRW + 2, kCH = kRH + 2;       // centres: 32 x 16
constexpr int kQW = kRW + 4, kQH = kRH + 4;       // points: 34 x 18
static_assert(kCW == 32 && kCH == 16, "thread maps below");

constexpr int kRegLds = 3 * kQH * (kQW + 1) + 6 * kCH * (kCW + 1) + 4;   // floats

// grid of regloss_fused_kernel: kRW x kRH own pixels per workgroup
inline dim3 reg_fused_grid(int H, int W) { return dim3((W + kRW - 1) / kRW, (H + kRH - 1) / kRH); }

// workgroup (bx, by) of a grid gx wide; `lds` = kRegLds floats
__device__ __forceinline__ void regloss_fused_body(RegArgs a, float* __restrict__ partial, float* __restrict__ d_allmap, int bx, int by, int gx,
                                                   float* __restrict__ lds)
{
    if (a.rays_slot) a.rays_d = *a.rays_slot;
    float (*s_p)[kQH][kQW + 1] = reinterpret_cast<float (*)[kQH][kQW + 1]>(lds);
    float (*s_g)[kCH][kCW + 1] = reinterpret_cast<float (*)[kCH][kCW + 1]>(lds + 3 * kQH * (kQW + 1));
    float* s_red = lds + 3 * kQH * (kQW + 1) + 6 * kCH * (kCW + 1);
    const int tid = threadIdx.x;
    const int x0 = bx * kRW, y0 = by * kRH;      // first own pixel
    const unsigned HW = (unsigned)a.H * (unsigned)a.W;
    const GlobalF am = (GlobalF)a.allmap, rd = (GlobalF)a.rays_d;
    const float ox = a.rays_o[0], oy = a.rays_o[1], oz = a.rays_o[2];
    {
        constexpr int kTrips = (kQW * kQH + 255) / 256;          // 3
        float d[kTrips], r0[kTrips], r1[kTrips], r2[kTrips];
#pragma unroll
        for (int t = 0; t < kTrips; t++) {
            const int i = min(tid + 256 * t, kQW * kQH - 1), r = i / kQW, c = i - r * kQW;
            const unsigned q = (unsigned)min(max(y0 + r - 2, 0), a.H - 1) * (unsigned)a.W + (unsigned)min(max(x0 + c - 2, 0), a.W - 1);
            d[t] = am[5 * HW + q]; r0[t] = rd[3 * q]; r1[t] = rd[3 * q + 1]; r2[t] = rd[3 * q + 2];
        }
#pragma unroll
        for (int t = 0; t < kTrips; t++) {
            const int i = tid + 256 * t, r = i / kQW, c = i - r * kQW;
            if (i < kQW * kQH) {       // points outside the image are only read by centres that are not interior (their vectors are 0)
                const float dc = clean_depth(d[t]);
                s_p[0][r][c] = dc * r0[t] + ox; s_p[1][r][c] = dc * r1[t] + oy; s_p[2][r][c] = dc * r2[t] + oz;
            }
        }
    }
    const int cx = tid & 31;
    float wv[9];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int k = 0; k < 3; k++) wv[3 * c + k] = a.wvt[4 * c + k];
    const float inv_hw = 1.0f / (float)HW;
    const float kn = -inv_hw * a.ln;
    // the centres' own planes and (for phase 3) the own pixels' ray and raw depth: issued before the barrier
    float al[2], n0[2], n1[2], n2[2], ds[2], q0[2], q1[2], q2[2], raw[2];
    bool own[2], interior[2];
    unsigned qq[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int cy = (tid >> 5) + 8 * t;
        const int x = x0 + cx - 1, y = y0 + cy - 1;
        own[t] = cx >= 1 && cx <= kRW && cy >= 1 && cy <= kRH && x < a.W && y < a.H;
        interior[t] = x >= 1 && y >= 1 && x < a.W - 1 && y < a.H - 1;
        qq[t] = (unsigned)min(max(y, 0), a.H - 1) * (unsigned)a.W + (unsigned)min(max(x, 0), a.W - 1);
        al[t] = am[HW + qq[t]]; n0[t] = am[2 * HW + qq[t]]; n1[t] = am[3 * HW + qq[t]]; n2[t] = am[4 * HW + qq[t]];
        ds[t] = am[6 * HW + qq[t]]; raw[t] = am[5 * HW + qq[t]];
        q0[t] = rd[3 * qq[t]]; q1[t] = rd[3 * qq[t] + 1]; q2[t] = rd[3 * qq[t] + 2];
    }
    __syncthreads();
    float val = 0.f;
    float gn[2][3];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int cy = (tid >> 5) + 8 * t;
        float ddx[3] = {0.f, 0.f, 0.f}, ddy[3] = {0.f, 0.f, 0.f};
        float dot = 0.f;
        gn[t][0] = gn[t][1] = gn[t][2] = 0.f;
        if (interior[t]) {
            // centre (cy, cx) is point (cy + 1, cx + 1) of the region
            float dx[3], dy[3], v[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                dx[c] = s_p[c][cy + 2][cx + 1] - s_p[c][cy][cx + 1];
                dy[c] = s_p[c][cy + 1][cx + 2] - s_p[c][cy + 1][cx];
            }
            v[0] = dx[1] * dy[2] - dx[2] * dy[1];
            v[1] = dx[2] * dy[0] - dx[0] * dy[2];
            v[2] = dx[0] * dy[1] - dx[1] * dy[0];
            const float L = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            const float denom = fmaxf(L, 1e-12f);
            const float n[3] = {v[0] / denom, v[1] / denom, v[2] / denom};
            float nw[3];
#pragma unroll
            for (int c = 0; c < 3; c++) nw[c] = n0[t] * wv[3 * c] + n1[t] * wv[3 * c + 1] + n2[t] * wv[3 * c + 2];   // n_view @ wvt[:3,:3].T
            const float inv = al[t] / denom;                                     // normalize(), then * alpha
#pragma unroll
            for (int c = 0; c < 3; c++) dot += nw[c] * v[c] * inv;
            // d / d rend_normal (view space): -lambda/HW * wvt[:3,:3]^T-rotated surf_normal
#pragma unroll
            for (int kk = 0; kk < 3; kk++) {
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < 3; c++) acc += wv[3 * c + kk] * (n[c] * al[t]);
                gn[t][kk] = kn * acc;
            }
            // d / d n (alpha is detached), then through F.normalize and the cross product
            const float dn[3] = {kn * nw[0] * al[t], kn * nw[1] * al[t], kn * nw[2] * al[t]};
            float dv[3];
            if (L >= 1e-12f) {
                const float nd = n[0] * dn[0] + n[1] * dn[1] + n[2] * dn[2];
#pragma unroll
                for (int c = 0; c < 3; c++) dv[c] = (dn[c] - n[c] * nd) / L;
            } else {
#pragma unroll
                for (int c = 0; c < 3; c++) dv[c] = dn[c] / 1e-12f;
            }
            ddx[0] = dy[1] * dv[2] - dy[2] * dv[1]; ddx[1] = dy[2] * dv[0] - dy[0] * dv[2]; ddx[2] = dy[0] * dv[1] - dy[1] * dv[0];   // dy x dv
            ddy[0] = dv[1] * dx[2] - dv[2] * dx[1]; ddy[1] = dv[2] * dx[0] - dv[0] * dx[2]; ddy[2] = dv[0] * dx[1] - dv[1] * dx[0];   // dv x dx
        }
#pragma unroll
        for (int c = 0; c < 3; c++) { s_g[c][cy][cx] = ddx[c]; s_g[3 + c][cy][cx] = ddy[c]; }
        if (own[t]) val += (a.ln * (1.f - dot) + a.ld * ds[t]) * inv_hw;
    }
    __syncthreads();
    typedef float __attribute__((address_space(1)))* GlobalW;
    const GlobalW out = (GlobalW)d_allmap;
#pragma unroll
    for (int t = 0; t < 2; t++) {
        if (!own[t]) continue;
        const int cy = (tid >> 5) + 8 * t;
        float g3[3];
#pragma unroll
        for (int c = 0; c < 3; c++) g3[c] = s_g[c][cy - 1][cx] - s_g[c][cy + 1][cx] + s_g[3 + c][cy][cx - 1] - s_g[3 + c][cy][cx + 1];
        const float r = raw[t];
        const bool finite = !(r != r || r == INFINITY || r == -INFINITY);        // nan_to_num has zero gradient there
        const unsigned q = qq[t];
        out[q] = 0.f; out[HW + q] = 0.f;
        out[2 * HW + q] = gn[t][0]; out[3 * HW + q] = gn[t][1]; out[4 * HW + q] = gn[t][2];
        out[5 * HW + q] = finite ? g3[0] * q0[t] + g3[1] * q1[t] + g3[2] * q2[t] : 0.f;
        out[6 * HW + q] = inv_hw * a.ld;
        out[7 * HW + q] = 0.f;
    }
    for (int d = 32; d >= 1; d >>= 1) val += __shfl_xor(val, d, 64);
    if ((tid & 63) == 0) s_red[tid >> 6] = val;
    __syncthreads();
    if (tid == 0) partial[by * gx + bx] = s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

__global__ void __launch_bounds__(256) regloss_fused_kernel(RegArgs a, float* __restrict__ partial, float* __restrict__ d_allmap)
{
    __shared__ float lds[kRegLds];
    regloss_fused_body(a, partial, d_allmap, blockIdx.x, blockIdx.y, gridDim.x, lds);
}

// Both forward halves of the loss in ONE launch (dgs_loss_forward_merged).  The photometric kernel (SSIM windows: FMA-bound with a
// store-heavy epilogue) and the regulariser kernel (three short phases between barriers: latency-bound) read different
// rasterizer outputs and write different buffers; launched one after the other each leaves the chip partly idle (1305 and 1566
// workgroups at 800 x 800: a second partial round of workgroups each) and pays its own launch gap.  Here the two kinds of
// workgroup alternate in one grid while both last, so that every CU holds both at once.
__global__ void __launch_bounds__(256) loss_fwd_merged_kernel(SsimFwdArgs A, Gauss g, int sgx, int sgy, int sgz, RegArgs a,
                                                              float* __restrict__ reg_partial, float* __restrict__ d_allmap, int rgx, int rgy)
{
    constexpr int kMergedLds = kSsimFwdLds > kRegLds ? kSsimFwdLds : kRegLds;
    __shared__ float lds[kMergedLds];
    const int ns = sgx * sgy * sgz, nr = rgx * rgy, both = 2 * min(ns, nr);
    const int bid = blockIdx.x;
    bool photo; int i;
    if (bid < both) { photo = !(bid & 1); i = bid >> 1; }
    else { photo = ns > nr; i = bid - both + min(ns, nr); }
    if (photo) {
        const int bz = i / (sgx * sgy), r = i - bz * (sgx * sgy), by = r / sgx, bx = r - by * sgx;
        ssim_fwd_body(A, g, bx, by, bz, sgx, sgy, sgz, lds);
    } else {
        const int by = i / rgx, bx = i - by * rgx;
        regloss_fused_body(a, reg_partial, d_allmap, bx, by, rgx, lds);
    }
}

}  // namespace
