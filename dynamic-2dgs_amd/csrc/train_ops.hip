// train_ops.hip -- the C entry points of libdgs_train_ops.so for gfx950 (include/dgs_train_ops.h): argument checks and
// launches, nothing else.  The kernels live in one header per family:
//   loss_kernels.h      SSIM / photometric loss, the regularisers, the merged loss forward, the loss combine
//   metric_kernels.h    image metrics of an evaluation run: squared error, SSIM and MS-SSIM sums per plane, the pooled pyramid level
//   knn_kernels.h       brute-force KNN and its two seeded refinements
//   skinning_kernels.h  control-node skinning, forward and backward, and the reduces of its gradient tables
//   step_kernels.h      step guard, view selection, flat Adam, densification statistics
//   node_mlp.h          the control-node MLP
//   train_common.h      error string, launch check
// The entry points below follow the same order.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/dgs_train_ops.h"
#include "knn_kernels.h"
#include "loss_kernels.h"
#include "metric_kernels.h"
#include "node_mlp.h"
#include "skinning_kernels.h"
#include "step_kernels.h"
#include "train_common.h"
#include "wave_reduce.h"

extern "C" {

int dgs_train_ops_abi_version(void) { return DGS_TRAIN_OPS_ABI_VERSION; }
const char* dgs_train_ops_last_error(void) { return g_err.c_str(); }

// ---- SSIM ---------------------------------------------------------------------------------------------------------------
int dgs_ssim_forward(int C, int H, int W, const float* img1, const float* img2, float* ssim_sum, float* dm_dmu1,
                     float* dm_dsigma1_sq, float* dm_dsigma12, void* stream)
{
    if (C <= 0 || H <= 0 || W <= 0 || !img1 || !img2 || !ssim_sum) return fail(-1, "dgs_ssim_forward: bad argument");
    if ((dm_dmu1 != nullptr) != (dm_dsigma1_sq != nullptr) || (dm_dmu1 != nullptr) != (dm_dsigma12 != nullptr))
        return fail(-1, "dgs_ssim_forward: pass all three derivative maps or none");
    const dim3 grid = ssim_grid(C, H, W);
    const SsimFwdArgs A{H, W, img1, img2, ssim_sum, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(ssim_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, A, gauss());
    return launched("ssim_fwd_kernel");
}

int dgs_ssim_backward(int C, int H, int W, const float* img1, const float* img2, const float* dm_dmu1,
                      const float* dm_dsigma1_sq, const float* dm_dsigma12, const float* dL_dmean, float* dL_dimg1,
                      void* stream)
{
    if (C <= 0 || H <= 0 || W <= 0 || !img1 || !img2 || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_dmean || !dL_dimg1)
        return fail(-1, "dgs_ssim_backward: bad argument");
    const dim3 grid = ssim_grid(C, H, W);
    const float inv_n = 1.0f / ((float)C * (float)H * (float)W);
    hipLaunchKernelGGL(ssim_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, H, W, inv_n, 0.f, img1, img2, gauss(), dm_dmu1, dm_dsigma1_sq,
                       dm_dsigma12, dL_dmean, dL_dimg1, (const float* const*)nullptr, CombineArgs{});
    return launched("ssim_bwd_kernel");
}

// ---- photometric loss: (1 - lambda) * mean|img - gt| + lambda * (1 - SSIM) (train_gui.py:292-296) ---------------------
size_t dgs_photo_blocks(int C, int H, int W) { const dim3 g = ssim_grid(C, H, W); return (size_t)g.x * g.y * g.z; }

int dgs_photo_forward(int C, int H, int W, const float* img, const float* gt, float* partials, float* dm_dmu1, float* dm_dsigma1_sq,
                      float* dm_dsigma12, const float* const* gt_slot, void* stream)
{
    if (C <= 0 || H <= 0 || W <= 0 || !img || !gt || !partials || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12)
        return fail(-1, "dgs_photo_forward: bad argument");
    const dim3 grid = ssim_grid(C, H, W);
    const SsimFwdArgs A{H, W, img, gt, nullptr, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, nullptr, partials, gt_slot};
    hipLaunchKernelGGL(ssim_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, A, gauss());
    return launched("ssim_fwd_kernel");
}

int dgs_photo_backward_combine_guard(int C, int H, int W, const float* img, const float* gt, const float* dm_dmu1, const float* dm_dsigma1_sq,
                                     const float* dm_dsigma12, float lambda_dssim, const float* g_loss, float* dL_dimg,
                                     const float* const* gt_slot, const float* photo_partials, long long nphoto, const float* reg_partials,
                                     long long nreg, float* loss_out, const int* guard_skip, float* guard_step_count, float* guard_status,
                                     float* guard_ring, int guard_ring_len, void* stream)
{
    if (guard_step_count && (!loss_out || !guard_status || (guard_ring && guard_ring_len <= 0)))
        return fail(-1, "dgs_photo_backward_combine_guard: the guard needs loss_out, status and a ring length");
    if (C <= 0 || H <= 0 || W <= 0 || !img || !gt || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !g_loss || !dL_dimg)
        return fail(-1, "dgs_photo_backward: bad argument");
    if (loss_out && (!photo_partials || !reg_partials || nphoto < 0 || nreg < 0)) return fail(-1, "dgs_photo_backward_combine: bad argument");
    const dim3 grid = ssim_grid(C, H, W);
    const float inv_n = 1.0f / ((float)C * (float)H * (float)W);
    CombineArgs c{photo_partials, (int)nphoto, reg_partials, (int)nreg, inv_n, lambda_dssim, loss_out,
                  guard_skip, guard_step_count, guard_status, guard_ring, guard_ring_len};
    hipLaunchKernelGGL(ssim_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, H, W, -lambda_dssim * inv_n,
                       (1.0f - lambda_dssim) * inv_n, img, gt, gauss(), dm_dmu1, dm_dsigma1_sq, dm_dsigma12, g_loss, dL_dimg, gt_slot, c);
    return launched("ssim_bwd_kernel");
}

int dgs_photo_backward_combine(int C, int H, int W, const float* img, const float* gt, const float* dm_dmu1, const float* dm_dsigma1_sq,
                               const float* dm_dsigma12, float lambda_dssim, const float* g_loss, float* dL_dimg, const float* const* gt_slot,
                               const float* photo_partials, long long nphoto, const float* reg_partials, long long nreg, float* loss_out,
                               void* stream)
{
    return dgs_photo_backward_combine_guard(C, H, W, img, gt, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, lambda_dssim, g_loss, dL_dimg, gt_slot,
                                            photo_partials, nphoto, reg_partials, nreg, loss_out, nullptr, nullptr, nullptr, nullptr, 0, stream);
}

int dgs_photo_backward(int C, int H, int W, const float* img, const float* gt, const float* dm_dmu1, const float* dm_dsigma1_sq,
                       const float* dm_dsigma12, float lambda_dssim, const float* g_loss, float* dL_dimg, const float* const* gt_slot,
                       void* stream)
{
    return dgs_photo_backward_combine(C, H, W, img, gt, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, lambda_dssim, g_loss, dL_dimg, gt_slot, nullptr, 0,
                                      nullptr, 0, nullptr, stream);
}

int dgs_loss_combine(const float* photo_partials, long long nphoto, const float* reg_partials, long long nreg, long long n,
                     float lambda_dssim, float* out, void* stream)
{
    if (!photo_partials || !reg_partials || !out || n <= 0 || nphoto < 0 || nreg < 0) return fail(-1, "dgs_loss_combine: bad argument");
    CombineArgs c{photo_partials, (int)nphoto, reg_partials, (int)nreg, 1.0f / (float)n, lambda_dssim, out, nullptr, nullptr, nullptr, nullptr, 0};
    hipLaunchKernelGGL(loss_combine_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, c);
    return launched("loss_combine_kernel");
}

// ---- regularisers, and both forward halves of the loss in one launch -----------------------------------------------------
size_t dgs_regloss_blocks(int H, int W) { const dim3 g = reg16_grid(H, W); return (size_t)g.x * g.y; }

int dgs_regloss_forward(int H, int W, const float* allmap, const float* rays_d, const float* rays_o, const float* wvt,
                        float lambda_normal, float lambda_dist, float* loss, void* stream)
{
    if (H <= 0 || W <= 0 || !allmap || !rays_d || !rays_o || !wvt || !loss) return fail(-1, "dgs_regloss_forward: bad argument");
    RegArgs a{H, W, allmap, rays_d, rays_o, wvt, lambda_normal, lambda_dist, nullptr, 0, nullptr};
    hipLaunchKernelGGL(regloss_fwd_kernel, reg16_grid(H, W), dim3(256), 0, (hipStream_t)stream, a, loss, (float*)nullptr);
    return launched("regloss_fwd_kernel");
}

int dgs_regloss_backward(int H, int W, const float* allmap, const float* rays_d, const float* rays_o, const float* wvt,
                         float lambda_normal, float lambda_dist, const float* g, float* d_allmap, void* stream)
{
    if (H <= 0 || W <= 0 || !allmap || !rays_d || !rays_o || !wvt || !g || !d_allmap) return fail(-1, "dgs_regloss_backward: bad argument");
    RegArgs a{H, W, allmap, rays_d, rays_o, wvt, lambda_normal, lambda_dist, nullptr, 0, nullptr};
    hipLaunchKernelGGL(regloss_bwd_kernel, reg16_grid(H, W), dim3(256), 0, (hipStream_t)stream, a, g, d_allmap);
    return launched("regloss_bwd_kernel");
}

int dgs_regloss_backward_slot(int H, int W, const float* allmap, const float* rays_d, const float* rays_o, const float* wvt,
                              float lambda_normal, float lambda_dist, const float* g, float* d_allmap, const float* const* rays_slot,
                              int write_all, void* stream)
{
    if (H <= 0 || W <= 0 || !allmap || (!rays_d && !rays_slot) || !rays_o || !wvt || !g || !d_allmap)
        return fail(-1, "dgs_regloss_backward_slot: bad argument");
    RegArgs a{H, W, allmap, rays_d, rays_o, wvt, lambda_normal, lambda_dist, rays_slot, write_all, nullptr};
    hipLaunchKernelGGL(regloss_bwd_kernel, reg16_grid(H, W), dim3(256), 0, (hipStream_t)stream, a, g, d_allmap);
    return launched("regloss_bwd_kernel");
}

int dgs_regloss_forward_partials(int H, int W, const float* allmap, const float* rays_d, const float* rays_o, const float* wvt,
                                 float lambda_normal, float lambda_dist, float* partials, const float* const* rays_slot, void* stream)
{
    return dgs_regloss_forward_partials_z(H, W, allmap, rays_d, rays_o, wvt, lambda_normal, lambda_dist, partials, rays_slot, nullptr, stream);
}

int dgs_regloss_forward_partials_z(int H, int W, const float* allmap, const float* rays_d, const float* rays_o, const float* wvt,
                                   float lambda_normal, float lambda_dist, float* partials, const float* const* rays_slot,
                                   float* zero_plane, void* stream)
{
    if (H <= 0 || W <= 0 || !allmap || (!rays_d && !rays_slot) || !rays_o || !wvt || !partials)
        return fail(-1, "dgs_regloss_forward_partials: bad argument");
    RegArgs a{H, W, allmap, rays_d, rays_o, wvt, lambda_normal, lambda_dist, rays_slot, 0, zero_plane};
    hipLaunchKernelGGL(regloss_fwd_kernel, reg16_grid(H, W), dim3(256), 0, (hipStream_t)stream, a, (float*)nullptr,
                       partials);
    return launched("regloss_fwd_kernel");
}

size_t dgs_regloss_fused_blocks(int H, int W) { const dim3 g = reg_fused_grid(H, W); return (size_t)g.x * g.y; }

int dgs_regloss_fused(int H, int W, const float* allmap, const float* rays_d, const float* rays_o, const float* wvt, float lambda_normal,
                      float lambda_dist, float* partials, float* d_allmap, const float* const* rays_slot, void* stream)
{
    if (H <= 0 || W <= 0 || !allmap || (!rays_d && !rays_slot) || !rays_o || !wvt || !partials || !d_allmap)
        return fail(-1, "dgs_regloss_fused: bad argument");
    if ((long long)H * W * 8 >= (1ll << 32)) return fail(-2, "dgs_regloss_fused: image too large for 32-bit offsets");
    RegArgs a{H, W, allmap, rays_d, rays_o, wvt, lambda_normal, lambda_dist, rays_slot, 1, nullptr};
    hipLaunchKernelGGL(regloss_fused_kernel, reg_fused_grid(H, W), dim3(256), 0, (hipStream_t)stream, a, partials,
                       d_allmap);
    return launched("regloss_fused_kernel");
}

int dgs_loss_forward_merged(int C, int H, int W, const float* img, const float* gt, float* photo_partials, float* dm_dmu1,
                            float* dm_dsigma1_sq, float* dm_dsigma12, const float* const* gt_slot, const float* allmap, const float* rays_d,
                            const float* rays_o, const float* wvt, float lambda_normal, float lambda_dist, float* reg_partials,
                            float* d_allmap, const float* const* rays_slot, void* stream)
{
    if (C <= 0 || H <= 0 || W <= 0 || !img || !gt || !photo_partials || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !allmap ||
        (!rays_d && !rays_slot) || !rays_o || !wvt || !reg_partials || !d_allmap)
        return fail(-1, "dgs_loss_forward_merged: bad argument");
    if ((long long)H * W * 8 >= (1ll << 32)) return fail(-2, "dgs_loss_forward_merged: image too large for 32-bit offsets");
    const dim3 sg = ssim_grid(C, H, W), rg = reg_fused_grid(H, W);
    const long long total = (long long)sg.x * sg.y * sg.z + (long long)rg.x * rg.y;
    if (total >= (1ll << 31)) return fail(-2, "dgs_loss_forward_merged: grid too large");
    const SsimFwdArgs A{H, W, img, gt, nullptr, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, nullptr, photo_partials, gt_slot};
    const RegArgs a{H, W, allmap, rays_d, rays_o, wvt, lambda_normal, lambda_dist, rays_slot, 1, nullptr};
    hipLaunchKernelGGL(loss_fwd_merged_kernel, dim3((unsigned)total), dim3(256), 0, (hipStream_t)stream, A, gauss(), (int)sg.x, (int)sg.y, C, a,
                       reg_partials, d_allmap, (int)rg.x, (int)rg.y);
    return launched("loss_fwd_merged_kernel");
}

// ---- image metrics of an evaluation run (metric_kernels.h) ----------------------------------------------------------------
int dgs_image_metrics_layout(int out[3])
{
    if (!out) return fail(-1, "dgs_image_metrics_layout: NULL pointer");
    out[0] = kTW; out[1] = kTH; out[2] = kMetricThreads;
    return 0;
}

// 0 = same (H x W outputs, zero padding), 1 = valid ((H - 10) x (W - 10) outputs); the output domain, or false
static bool metric_domain(int H, int W, int window, int* OH, int* OW)
{
    if (H < 1 || W < 1 || (window != 0 && window != 1)) return false;
    *OH = window ? H - 2 * kR : H; *OW = window ? W - 2 * kR : W;
    return *OH >= 1 && *OW >= 1;
}

size_t dgs_image_metrics_scratch_floats(int B, int C, int H, int W, int window)
{
    int OH, OW;
    if (B < 1 || C < 1 || !metric_domain(H, W, window, &OH, &OW)) return 0;
    const dim3 g = metric_grid(1, OH, OW);
    return (size_t)B * C * g.x * g.y * 3;
}

int dgs_image_metrics(int B, int C, int H, int W, const float* pred, const float* gt, int window, int quantize, double* out,
                      float* pooled_pred, float* pooled_gt, float* scratch, void* stream)
{
    if (B < 1 || C < 1 || (long long)B * C > 65535) return fail(-1, "dgs_image_metrics: B * C must be in [1, 65535] (grid z limit)");
    if (H < 1 || W < 1) return fail(-1, "dgs_image_metrics: H and W must be at least 1");
    if (window != 0 && window != 1) return fail(-1, "dgs_image_metrics: window must be 0 (same) or 1 (valid)");
    int OH, OW;
    if (!metric_domain(H, W, window, &OH, &OW)) return fail(-1, "dgs_image_metrics: the valid window needs H >= 11 and W >= 11");
    if (!pred || !gt || !out || !scratch) return fail(-1, "dgs_image_metrics: NULL pointer");
    if ((pooled_pred != nullptr) != (pooled_gt != nullptr)) return fail(-1, "dgs_image_metrics: pass both pooled planes or none");
    if ((long long)H * W >= (1ll << 31)) return fail(-2, "dgs_image_metrics: plane too large for 32-bit offsets");
    const dim3 grid = metric_grid(B * C, OH, OW);
    if (grid.y > 65535) return fail(-2, "dgs_image_metrics: too many tile rows for the grid");
    const MetricArgs A{H, W, OH, OW, window ? 0 : kR, quantize ? 1 : 0, pred, gt, scratch, pooled_pred, pooled_gt, (H + 1) / 2, (W + 1) / 2};
    hipLaunchKernelGGL(image_metrics_kernel, grid, dim3(kMetricThreads), 0, (hipStream_t)stream, A, gauss());
    if (int e = launched("image_metrics_kernel")) return e;
    hipLaunchKernelGGL(image_metrics_combine_kernel, dim3(B * C), dim3(kMetricThreads), 0, (hipStream_t)stream, (const float*)scratch,
                       (int)(grid.x * grid.y), out);
    return launched("image_metrics_combine_kernel");
}

// ---- KNN ----------------------------------------------------------------------------------------------------------------
int dgs_knn_points(int N, int M, int D, int K, const float* x, const float* nodes, long long* idx, float* dist2,
                   void* stream)
{
    if (N < 0 || M <= 0 || D < 1 || D > kKnnDpad || K < 1 || K > 4 || K > M) return fail(-1, "dgs_knn_points: bad argument");
    if (N == 0) return 0;
    if (!x || !nodes || !idx) return fail(-1, "dgs_knn_points: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    return dispatch_K(K, [&](auto k) { return launch_knn<decltype(k)::value>(N, M, D, x, nodes, idx, dist2, s); });
}

int dgs_knn_points2(int N, int M, int D1, int D2, int K, const float* x1, const float* x2, int x2_stride, const float* nodes,
                    long long* idx, float* dist2, void* stream)
{
    const int D = D1 + D2;
    if (N < 0 || M <= 0 || D1 < 1 || D2 < 1 || D > kKnnDpad || K < 1 || K > 4 || K > M) return fail(-1, "dgs_knn_points2: bad argument");
    if (N == 0) return 0;
    if (!x1 || !x2 || !nodes || !idx) return fail(-1, "dgs_knn_points2: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    return dispatch_K(K, [&](auto k) { return launch_knn<decltype(k)::value>(N, M, D, x1, nodes, idx, dist2, s, x2, D1, x2_stride); });
}

int dgs_knn_refine_mode(int N, int M, int D1, int D2, int K, const float* x1, const float* x2, int x2_stride, const float* nodes,
                        long long* idx, int mode, void* stream)
{
    const int D = D1 + D2;
    if (mode != 0 && mode != 1) return fail(-1, "dgs_knn_refine: mode must be 0 (3-D culling) or 1 (matrix cores)");
    if (N < 0 || M <= 0 || D1 < 3 || D2 < 0 || D > kKnnDpad || K < 1 || K > 4 || K > M) return fail(-1, "dgs_knn_refine: bad argument");
    if (M > 2048) return fail(-2, "dgs_knn_refine: more than 2048 nodes (use dgs_knn_points)");
    if (N == 0) return 0;
    if (!x1 || (D2 > 0 && !x2) || !nodes || !idx) return fail(-1, "dgs_knn_refine: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    const float* xb = D2 > 0 ? x2 : nullptr;
    return dispatch_K(K, [&](auto k) { return launch_knn_refine<decltype(k)::value>(N, M, D, x1, nodes, idx, s, xb, D1, x2_stride, mode == 1); });
}

int dgs_knn_refine(int N, int M, int D1, int D2, int K, const float* x1, const float* x2, int x2_stride, const float* nodes,
                   long long* idx, void* stream)
{
    return dgs_knn_refine_mode(N, M, D1, D2, K, x1, x2, x2_stride, nodes, idx, 0, stream);
}

// ---- control-node skinning -----------------------------------------------------------------------------------------------
int dgs_lbs_supported(int M, int H) { return H >= 0 && H <= kLbsHmax && M > 0 && M <= 4 * kLbsBwdThreads && lbs_bwd_lds_bytes(M, H) <= 160 * 1024; }
size_t dgs_lbs_scratch_bytes(int M, int H) { return (size_t)kLbsBlocks * (size_t)M * (size_t)(kLbsAttr + H + 2) * sizeof(float); }

static int lbs_check(int N, int M, int H)
{
    if (N < 0 || M <= 0 || H < 0 || H > kLbsHmax) return fail(-1, "dgs_lbs: bad sizes");
    return 0;
}

int dgs_lbs_forward(int N, int M, int H, const float* x, const float* feature, int feature_stride, const long long* idx,
                    const float* ntab, const float* attrs, const float* mask, float* d_xyz, float* d_rot, float* d_scale,
                    void* stream)
{
    if (int e = lbs_check(N, M, H)) return e;
    if (N == 0) return 0;
    const LbsArgs a = lbs_args_table(N, M, H, x, feature, feature_stride, idx, ntab, attrs, mask);
    hipLaunchKernelGGL(lbs_fwd_kernel<false>, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, d_xyz, d_rot, d_scale,
                       AsmArgs{});
    return launched("lbs_fwd_kernel");
}

int dgs_lbs_backward(int N, int M, int H, const float* x, const float* feature, int feature_stride, const long long* idx,
                     const float* ntab, const float* attrs, const float* mask, const float* g_xyz, const float* g_rot,
                     const float* g_scale, float* g_feature, float* g_ntab, float* g_attrs, void* scratch, void* stream)
{
    if (int e = lbs_check(N, M, H)) return e;
    const int G = kLbsAttr + H + 2;
    const size_t lds = lbs_bwd_lds_bytes(M, H);
    if (lds > 160 * 1024 || M > 4 * kLbsBwdThreads) return fail(-2, "dgs_lbs_backward: node tables do not fit the 160 KB of LDS");
    if (!scratch) return fail(-1, "dgs_lbs_backward: scratch is NULL");
    const LbsArgs a = lbs_args_table(N, M, H, x, feature, feature_stride, idx, ntab, attrs, mask);
    const int chunk = (N + kLbsBlocks - 1) / kLbsBlocks;
    hipLaunchKernelGGL((lbs_bwd_kernel<false, false>), dim3(kLbsBlocks), dim3(kLbsBwdThreads), lds, (hipStream_t)stream, a, g_xyz, g_rot, g_scale,
                       g_feature, H, 0, (float*)scratch, chunk > 0 ? chunk : 1, AsmArgs{});
    hipLaunchKernelGGL(lbs_reduce_kernel, dim3((M * G + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)scratch, M, H,
                       g_ntab, g_attrs, kLbsBlocks);
    return launched("lbs_bwd_kernel");
}

// ---- deformation + activations in one pass (dgs_deform_*) ------------------------------------------------------------
int dgs_deform_forward(int N, int M, int H, const float* xyz, const float* feature, int feature_stride, const long long* idx,
                       const float* nodes, const float* node_radius_raw, const float* node_weight_raw, const float* attrs,
                       const float* mask, const float* scaling_raw, const float* rotation_raw, const float* opacity_raw,
                       float* means3D, float* scales, float* rotations, float* opacity, void* stream)
{
    if (int e = lbs_check(N, M, H)) return e;
    if (N == 0) return 0;
    if (!xyz || !feature || !idx || !nodes || !node_radius_raw || !node_weight_raw || !attrs || !scaling_raw || !rotation_raw ||
        !opacity_raw || !means3D || !scales || !rotations || !opacity)
        return fail(-1, "dgs_deform_forward: NULL pointer");
    const LbsArgs a = lbs_args_raw(N, M, H, xyz, feature, feature_stride, idx, nodes, node_radius_raw, node_weight_raw, attrs, mask);
    AsmArgs s = asm_surfel_args(scaling_raw, rotation_raw, opacity_raw);
    s.means3D = means3D; s.scales = scales; s.rotations = rotations; s.opacity = opacity;
    hipLaunchKernelGGL(lbs_fwd_kernel<true>, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, (float*)nullptr,
                       (float*)nullptr, (float*)nullptr, s);
    return launched("lbs_fwd_kernel<asm>");
}

int dgs_deform_backward(int N, int M, int H, const float* xyz, const float* feature, int feature_stride, const long long* idx,
                        const float* nodes, const float* node_radius_raw, const float* node_weight_raw, const float* attrs,
                        const float* mask, const float* scaling_raw, const float* rotation_raw, const float* opacity_raw,
                        const float* g_means3D, const float* g_scales, const float* g_rotations, const float* g_opacity,
                        float* g_xyz, float* g_scaling_raw, float* g_rotation_raw, float* g_opacity_raw, float* g_feature,
                        float* g_nodes, float* g_radius_raw, float* g_weight_raw, float* g_attrs, int accumulate, void* scratch,
                        void* stream)
{
    if (int e = lbs_check(N, M, H)) return e;
    const int G = kLbsAttr + H + 2;
    const size_t lds = lbs_bwd_lds_bytes(M, H);
    if (lds > 160 * 1024 || M > 4 * kLbsBwdThreads) return fail(-2, "dgs_deform_backward: node tables do not fit the 160 KB of LDS");
    // an empty surfel set (N == 0: the trainer prunes) has no per-surfel arrays; the node gradients are still produced (all zero)
    if (!scratch || !g_nodes || !g_radius_raw || !g_weight_raw || !g_attrs ||
        (N > 0 && (!g_means3D || !g_scales || !g_rotations || !g_opacity || !g_xyz || !g_scaling_raw || !g_rotation_raw ||
                   !g_opacity_raw || !g_feature)))
        return fail(-1, "dgs_deform_backward: NULL pointer");
    const LbsArgs a = lbs_args_raw(N, M, H, xyz, feature, feature_stride, idx, nodes, node_radius_raw, node_weight_raw, attrs, mask);
    AsmArgs s = asm_surfel_args(scaling_raw, rotation_raw, opacity_raw);
    s.g_means3D = g_means3D; s.g_scales = g_scales; s.g_rotations = g_rotations; s.g_opacity = g_opacity;
    s.g_xyz = g_xyz; s.g_scaling_raw = g_scaling_raw; s.g_rotation_raw = g_rotation_raw; s.g_opacity_raw = g_opacity_raw;
    if (accumulate & 2) {
        // coherent variant (surfels stored by nearest node): one zeroed [M][G] table, wave-level sums, global atomics
        // accumulate bit 2 (value 4): `scratch` is a persistent table that is zero on entry and must be zero on exit
        const bool persistent = (accumulate & 4) != 0;
        const bool fixed = (accumulate & 16) != 0;   // bit 4: 64-bit fixed-point table, integer atomics (order-free sums)
        if (!persistent) {
            const hipError_t me = hipMemsetAsync(scratch, 0, (size_t)M * G * (fixed ? sizeof(unsigned long long) : sizeof(float)), (hipStream_t)stream);
            if (me != hipSuccess) return fail(-4, std::string("dgs_deform_backward: ") + hipGetErrorString(me));
        }
        auto kern = fixed ? (H == 8 ? lbs_bwd_kernel<true, true, 8, true> : lbs_bwd_kernel<true, true, 0, true>)
                          : (H == 8 ? lbs_bwd_kernel<true, true, 8> : lbs_bwd_kernel<true, true, 0>);   // the trainer's hyper_dim, specialised
        if (N > 0)   // an empty grid is a launch error; the memset above and the reduce below still run
            hipLaunchKernelGGL(kern, dim3((N + kCohThreads - 1) / kCohThreads), dim3(kCohThreads), 0, (hipStream_t)stream, a,
                               (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, g_feature, feature_stride, accumulate & 1,
                               (float*)scratch, kCohThreads, s);
        if (!(accumulate & 8))      // bit 3: the caller reduces the table later (dgs_deform_reduce), e.g. on another stream
            hipLaunchKernelGGL(lbs_reduce_raw_kernel, dim3((M * G + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)scratch, M, H,
                               node_radius_raw, node_weight_raw, g_nodes, g_radius_raw, g_weight_raw, g_attrs, accumulate & 1, 1,
                               persistent ? (float*)scratch : (float*)nullptr, fixed ? 1 : 0);
    } else {
        if (accumulate & 16) return fail(-1, "dgs_deform_backward: the fixed-point table (bit 4) needs the coherent variant (bit 1)");
        if (accumulate & 8) return fail(-1, "dgs_deform_backward: the deferred reduce (bit 3) needs the coherent variant (bit 1)");
        const int chunk = (N + kLbsBlocks - 1) / kLbsBlocks;
        hipLaunchKernelGGL((lbs_bwd_kernel<true, false>), dim3(kLbsBlocks), dim3(kLbsBwdThreads), lds, (hipStream_t)stream, a, (const float*)nullptr,
                           (const float*)nullptr, (const float*)nullptr, g_feature, feature_stride, accumulate & 1, (float*)scratch,
                           chunk > 0 ? chunk : 1, s);
        hipLaunchKernelGGL(lbs_reduce_raw_kernel, dim3((M * G + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)scratch, M, H,
                           node_radius_raw, node_weight_raw, g_nodes, g_radius_raw, g_weight_raw, g_attrs, accumulate & 1, kLbsBlocks,
                           (float*)nullptr);
    }
    return launched("lbs_bwd_kernel<asm>");
}

int dgs_deform_reduce(int M, int H, const float* node_radius_raw, const float* node_weight_raw, float* g_nodes, float* g_radius_raw,
                      float* g_weight_raw, float* g_attrs, int accumulate, void* scratch, void* stream)
{
    if (M <= 0 || H < 0 || H > kLbsHmax || !scratch || !node_radius_raw || !node_weight_raw || !g_nodes || !g_radius_raw || !g_weight_raw || !g_attrs)
        return fail(-1, "dgs_deform_reduce: bad argument");
    const int G = kLbsAttr + H + 2;
    hipLaunchKernelGGL(lbs_reduce_raw_kernel, dim3((M * G + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)scratch, M, H,
                       node_radius_raw, node_weight_raw, g_nodes, g_radius_raw, g_weight_raw, g_attrs, accumulate & 1, 1,
                       (accumulate & 4) ? (float*)scratch : (float*)nullptr, (accumulate & 16) ? 1 : 0);
    return launched("lbs_reduce_raw_kernel");
}

// ---- flat Adam, step guard, view selection -------------------------------------------------------------------------------
size_t dgs_adam_plan_bytes(long long total) { return (size_t)(total / kAdamChunk + kAdamSeg + 1) * sizeof(int2); }

int dgs_adam_plan(int nseg, const long long* offsets, void* plan, void* stream)
{
    if (nseg <= 0 || nseg > kAdamSeg || !offsets || !plan) return fail(-1, "dgs_adam_plan: bad argument");
    std::vector<int2> host;
    for (int s = 0; s < nseg; s++)
        for (long long b = 0; b < offsets[s + 1] - offsets[s]; b += kAdamChunk) host.push_back(make_int2(s, (int)b));
    if (host.empty()) return 0;
    hipError_t e = hipMemcpyAsync(plan, host.data(), host.size() * sizeof(int2), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);  // `host` dies at return
    if (e != hipSuccess) return fail(-4, std::string("dgs_adam_plan: ") + hipGetErrorString(e));
    return 0;
}

int dgs_adam_step(int nseg, float* const* params, const long long* offsets, const float* lrs, const float* grad, float* exp_avg,
                  float* exp_avg_sq, const float* step_count, float beta1, float beta2, float eps, const void* plan, void* stream)
{
    return dgs_adam_step_pattern(nseg, params, offsets, lrs, nullptr, nullptr, nullptr, grad, exp_avg, exp_avg_sq, step_count, beta1,
                                 beta2, eps, plan, stream);
}

int dgs_adam_step_pattern(int nseg, float* const* params, const long long* offsets, const float* lrs, const float* lrs2,
                          const int* periods, const int* splits, const float* grad, float* exp_avg, float* exp_avg_sq,
                          const float* step_count, float beta1, float beta2, float eps, const void* plan, void* stream)
{
    return dgs_adam_step_sched(nseg, params, offsets, lrs, lrs2, periods, splits, nullptr, nullptr, 0.0f, 1.0f, grad, exp_avg, exp_avg_sq,
                               step_count, beta1, beta2, eps, plan, stream);
}

int dgs_adam_step_sched(int nseg, float* const* params, const long long* offsets, const float* lrs, const float* lrs2,
                        const int* periods, const int* splits, const float* lrs_final, const float* sched_steps, float sched_t0,
                        float grad_scale, const float* grad, float* exp_avg, float* exp_avg_sq, const float* step_count, float beta1, float beta2,
                        float eps, const void* plan, void* stream)
{
    return dgs_adam_step_guarded(nseg, params, offsets, lrs, lrs2, periods, splits, lrs_final, sched_steps, sched_t0, grad_scale, grad,
                                 exp_avg, exp_avg_sq, step_count, beta1, beta2, eps, plan, nullptr, stream);
}

int dgs_adam_step_guarded(int nseg, float* const* params, const long long* offsets, const float* lrs, const float* lrs2,
                          const int* periods, const int* splits, const float* lrs_final, const float* sched_steps, float sched_t0,
                          float grad_scale, const float* grad, float* exp_avg, float* exp_avg_sq, const float* step_count, float beta1,
                          float beta2, float eps, const void* plan, const int* skip, void* stream)
{
    return dgs_adam_step_zero(nseg, params, offsets, lrs, lrs2, periods, splits, lrs_final, sched_steps, sched_t0, grad_scale,
                              const_cast<float*>(grad), 0, exp_avg, exp_avg_sq, step_count, beta1, beta2, eps, plan, skip, stream);
}

int dgs_adam_step_zero(int nseg, float* const* params, const long long* offsets, const float* lrs, const float* lrs2,
                       const int* periods, const int* splits, const float* lrs_final, const float* sched_steps, float sched_t0,
                       float grad_scale, float* grad, int zero_grad, float* exp_avg, float* exp_avg_sq, const float* step_count,
                       float beta1, float beta2, float eps, const void* plan, const int* skip, void* stream)
{
    return dgs_adam_step_origin(nseg, params, offsets, lrs, lrs2, periods, splits, lrs_final, sched_steps, sched_t0, nullptr, grad_scale, grad,
                                zero_grad, exp_avg, exp_avg_sq, step_count, beta1, beta2, eps, plan, skip, stream);
}

int dgs_adam_step_origin(int nseg, float* const* params, const long long* offsets, const float* lrs, const float* lrs2,
                         const int* periods, const int* splits, const float* lrs_final, const float* sched_steps, float sched_t0,
                         const float* step_origins, float grad_scale, float* grad, int zero_grad, float* exp_avg, float* exp_avg_sq,
                         const float* step_count, float beta1, float beta2, float eps, const void* plan, const int* skip, void* stream)
{
    return dgs_adam_step_sum2(nseg, params, offsets, lrs, lrs2, periods, splits, lrs_final, sched_steps, sched_t0, step_origins, grad_scale, grad,
                              nullptr, zero_grad, exp_avg, exp_avg_sq, step_count, beta1, beta2, eps, plan, skip, stream);
}

int dgs_adam_step_sum2(int nseg, float* const* params, const long long* offsets, const float* lrs, const float* lrs2,
                       const int* periods, const int* splits, const float* lrs_final, const float* sched_steps, float sched_t0,
                       const float* step_origins, float grad_scale, float* grad, const float* grad2, int zero_grad, float* exp_avg,
                       float* exp_avg_sq, const float* step_count, float beta1, float beta2, float eps, const void* plan, const int* skip,
                       void* stream)
{
    if (grad2 && zero_grad) return fail(-1, "dgs_adam_step_sum2: zero_grad clears the first buffer only; clear both yourself");
    if ((lrs_final != nullptr) != (sched_steps != nullptr)) return fail(-1, "dgs_adam_step_sched: pass lrs_final and sched_steps together");
    if (nseg <= 0 || nseg > kAdamSeg || !params || !offsets || !lrs || !grad || !exp_avg || !exp_avg_sq || !step_count || !plan)
        return fail(-1, "dgs_adam_step: bad argument");
    if ((lrs2 != nullptr) != (periods != nullptr) || (lrs2 != nullptr) != (splits != nullptr))
        return fail(-1, "dgs_adam_step_pattern: pass lrs2, periods and splits together");
    AdamSegs sg;
    for (int s = 0; s < nseg; s++) {
        sg.p[s] = params[s]; sg.off[s] = offsets[s]; sg.lr[s] = lrs[s];
        sg.lr2[s] = lrs2 ? lrs2[s] : lrs[s];
        sg.period[s] = periods ? periods[s] : 0;
        sg.split[s] = splits ? splits[s] : 0;
        if (sg.period[s] < 0 || sg.split[s] < 0) return fail(-1, "dgs_adam_step_pattern: negative period / split");
        sg.lr_final[s] = lrs_final ? lrs_final[s] : lrs[s];
        sg.sched_steps[s] = sched_steps ? sched_steps[s] : 0.0f;
        sg.t_origin[s] = step_origins ? step_origins[s] : 0.0f;
        // (a NEGATIVE origin is a parameter that arrives with steps already taken elsewhere: the deformation model's optimiser runs on
        // from the node pre-training stage, Trainer.adopt_deform_state)
        if (sg.t_origin[s] != sg.t_origin[s]) return fail(-1, "dgs_adam_step_origin: step origin is NaN");
        if (sg.sched_steps[s] > 0.0f && !(lrs[s] > 0.0f && sg.lr_final[s] > 0.0f))
            return fail(-1, "dgs_adam_step_sched: a scheduled segment needs positive initial and final rates");
    }
    sg.sched_t0 = sched_t0;
    sg.gscale = grad_scale;
    sg.zero_grad = zero_grad ? 1 : 0;
    sg.off[nseg] = offsets[nseg];
    const long long nb = adam_blocks(nseg, offsets);
    if (nb == 0) return 0;
    static const int nt = getenv("DGS_ADAM_NT") ? atoi(getenv("DGS_ADAM_NT")) : 1;   // default 1: -0.9 % per step (0.760 against 0.767 ms, three pairs); 2: noise
    // grid cap: 16 workgroups per CU (two rounds of resident workgroups) walk the plan -- the surfel update beside the node-MLP
    // backward chain: 0.754 against 0.763 ms per step (five pairs; 1024: +-0, 2048: 0.756, 6144 / 8192: +-0); DGS_ADAM_WGS=0: uncapped
    static const long long cap = getenv("DGS_ADAM_WGS") ? atoll(getenv("DGS_ADAM_WGS")) : 4096;
    const unsigned grid = (unsigned)(cap > 0 && cap < nb ? cap : nb);
    const auto kern = nt == 2 ? adam_kernel<2> : (nt == 1 ? adam_kernel<1> : adam_kernel<0>);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, (hipStream_t)stream, sg, (const int2*)plan, (int)nb, grad, exp_avg, exp_avg_sq,
                       step_count, beta1, beta2, eps, skip, grad2);
    return launched("adam_kernel");
}

int dgs_select_row(const float* table, int nrows, int row_floats, int* counter, int* override_, int stride, int offset, float* row_out, void* stream)
{
    if (!table || !counter || !override_ || !row_out || nrows <= 0 || row_floats <= 0 || stride <= 0 || offset < 0)
        return fail(-1, "dgs_select_row: bad argument");
    const mlp::SelectArgs q{table, nrows, row_floats, counter, override_, stride, offset, row_out};
    hipLaunchKernelGGL(select_row_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, q);
    return launched("select_row_kernel");
}

int dgs_step_guard(const int* skip, float* step_count, float* status, float* host_ring, int ring_len, const float* loss, void* stream)
{
    if (!step_count || !status || (host_ring && ring_len <= 0)) return fail(-1, "dgs_step_guard: bad argument");
    hipLaunchKernelGGL(step_guard_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, skip, step_count, status, host_ring, ring_len, loss);
    return launched("step_guard_kernel");
}

// ---- control-node MLP (node_mlp.h) ---------------------------------------------------------------------------------
size_t dgs_mlp_packed_floats(void) { return mlp::kPackedFloats; }
size_t dgs_mlp_saved_floats(int M) { return mlp::sv_total(M); }
size_t dgs_mlp_scratch_floats(int M) { return mlp::sc_total(M); }

// params / grads: host arrays of 28 device pointers: (W, b) of T1, T2, L0..L7, local_rotation, warp, rotation, scaling
static const int kHeadRows[4] = {4, 3, 4, 2};

int dgs_mlp_forward(int M, const float* x, int x_stride, const float* t, int t_stride, const float* const* params,
                    const float* rot_bias, float* packed, float* saved, float* attrs, void* stream)
{
    return dgs_mlp_forward_select(M, x, x_stride, t, t_stride, params, rot_bias, packed, saved, attrs, nullptr, 0, 0, nullptr, nullptr, 1, 0,
                                  nullptr, stream);
}

int dgs_mlp_forward_select(int M, const float* x, int x_stride, const float* t, int t_stride, const float* const* params,
                           const float* rot_bias, float* packed, float* saved, float* attrs, const float* table, int nrows, int row_floats,
                           int* counter, int* override_, int stride, int offset, float* row_out, void* stream)
{
    if (M <= 0 || M % 64) return fail(-1, "dgs_mlp_forward: M must be a positive multiple of 64");
    if (table && (!counter || !override_ || !row_out || nrows <= 0 || row_floats <= 0 || stride <= 0 || offset < 0))
        return fail(-1, "dgs_mlp_forward_select: bad view table arguments");
    if (!x || !t || !params || !packed || !saved || !attrs) return fail(-1, "dgs_mlp_forward: null pointer");
    mlp::Weights w{};
    for (int l = 0; l < 10; l++) { w.W[l] = params[2 * l]; w.b[l] = params[2 * l + 1]; }
    int r = 0;
    for (int h = 0; h < 4; h++)
        for (int k = 0; k < kHeadRows[h]; k++, r++) { w.hw[r] = params[20 + 2 * h] + (size_t)k * mlp::kW; w.hb[r] = params[21 + 2 * h] + k; }
    for (; r < 16; r++) { w.hw[r] = w.hw[0]; w.hb[r] = w.hb[0]; }
    hipStream_t s = (hipStream_t)stream;
    int nthreads = mlp::kFwdVecs + mlp::kBwdVecs;   // one thread per float4 of the two operand arrays
    const mlp::SelectArgs sel{table, nrows, row_floats, counter, override_, stride, offset, row_out};
    hipLaunchKernelGGL(mlp::mlp_pack_kernel, dim3((nthreads + 255) / 256 + (table ? 1 : 0)), dim3(256), 0, s, w, reinterpret_cast<float4*>(packed), sel);
    mlp::FwdArgs a{};
    a.M = M; a.x = x; a.x_stride = x_stride; a.t = t; a.t_stride = t_stride;
    a.wp = reinterpret_cast<const float4*>(packed);
    a.bias = packed + mlp::kBiasOff;
    a.saved = saved; a.attrs = attrs;
    for (int i = 0; i < 4; i++) a.rot_bias[i] = rot_bias ? rot_bias[i] : 0.f;
    hipLaunchKernelGGL(mlp::mlp_fwd_kernel, dim3(M / mlp::kRows), dim3(mlp::kThreads), 0, s, a);
    return launched("dgs_mlp_forward", -2);
}

int dgs_mlp_backward(int M, const float* g_attrs, const float* packed, const float* saved, float* scratch, float* const* grads,
                     int accumulate, void* stream)
{
    return dgs_mlp_backward_reduce(M, const_cast<float*>(g_attrs), packed, saved, scratch, grads, accumulate, 0, nullptr, nullptr, nullptr, nullptr,
                                   nullptr, 0, nullptr, stream);
}

int dgs_mlp_backward_reduce(int M, float* g_attrs, const float* packed, const float* saved, float* scratch, float* const* grads,
                            int accumulate, int H, const float* node_radius_raw, const float* node_weight_raw, float* g_nodes,
                            float* g_radius_raw, float* g_weight_raw, int reduce_flags, void* lbs_table, void* stream)
{
    if (M <= 0 || M % 64) return fail(-1, "dgs_mlp_backward: M must be a positive multiple of 64");
    if (!g_attrs || !packed || !saved || !scratch || !grads) return fail(-1, "dgs_mlp_backward: null pointer");
    if (lbs_table && (H < 0 || H > kLbsHmax || !node_radius_raw || !node_weight_raw || !g_nodes || !g_radius_raw || !g_weight_raw))
        return fail(-1, "dgs_mlp_backward_reduce: bad argument");
    static_assert(kLbsAttr == mlp::kHeads, "the node table's attribute columns are the MLP's outputs");
    hipStream_t s = (hipStream_t)stream;
    mlp::BwdArgs b{};
    b.M = M; b.g_attrs = g_attrs; b.saved = saved; b.scratch = scratch;
    if (lbs_table)   // flags as dgs_deform_reduce: bit 0 add to the gradients, bit 2 leave the table zeroed
        b.fold = mlp::ReduceFold{(float*)lbs_table, kLbsAttr + H + 2, H, node_radius_raw, node_weight_raw, g_nodes, g_radius_raw, g_weight_raw,
                                 g_attrs, reduce_flags & 1, (reduce_flags & 4) ? 1 : 0, (reduce_flags & 16) ? 1 : 0};
    b.wq = reinterpret_cast<const float4*>(packed) + (size_t)mlp::kFwdVecs;
    hipLaunchKernelGGL(mlp::mlp_bwd_kernel, dim3(M / mlp::kRows), dim3(mlp::kThreads), 0, s, b);

    mlp::WgArgs g{};
    g.M = M; g.accumulate = accumulate;
    int r = 0;
    for (int h = 0; h < 4; h++)
        for (int k = 0; k < kHeadRows[h]; k++, r++) { g.hw[r] = grads[20 + 2 * h] + (size_t)k * mlp::kW; g.hb[r] = grads[21 + 2 * h] + k; }
    for (; r < 16; r++) { g.hw[r] = g.hw[0]; g.hb[r] = g.hb[0]; }
    int nd = 0, block = 0;
    auto add = [&](const float* dz, int dzs, int out, const float* x, int xs, int in, float* dw, int dws, float* db) {
        mlp::WgDesc& d = g.d[nd++];
        d.dz = dz; d.dz_stride = dzs; d.out = out; d.x = x; d.x_stride = xs; d.in = in; d.dw = dw; d.dw_stride = dws; d.db = db;
        d.iblocks = (in + mlp::kWgTileI - 1) / mlp::kWgTileI;
        d.ntiles = ((out + mlp::kWgTileJ - 1) / mlp::kWgTileJ) * d.iblocks;
    };
    const int W = mlp::kW;
    auto Hs = [&](int l) { return saved + mlp::sv_h(M, l); };
    auto dZ = [&](int l) { return scratch + mlp::sc_dz(M, l); };
    add(g_attrs, mlp::kHeads, mlp::kHeads, Hs(7), W, W, nullptr, W, nullptr);                          // heads
    for (int l = 7; l >= 1; l--) {
        float* gw = grads[2 * (l + 2)];
        float* gb = grads[2 * (l + 2) + 1];
        if (l == 5) {
            add(dZ(5), W, W, saved + mlp::sv_inp(M), mlp::kInPad, mlp::kIn, gw, mlp::kIn + W, gb);    // [inp | .]
            add(dZ(5), W, W, Hs(4), W, W, gw + mlp::kIn, mlp::kIn + W, nullptr);                       // [. | H4]
        } else {
            add(dZ(l), W, W, Hs(l - 1), W, W, gw, W, gb);
        }
    }
    add(dZ(0), W, W, saved + mlp::sv_inp(M), mlp::kInPad, mlp::kIn, grads[4], mlp::kIn, grads[5]);   // L0
    add(scratch + mlp::sc_dt2(M), 32, mlp::kTOut, saved + mlp::sv_t1(M), W, W, grads[2], W, grads[3]);        // time net 2
    add(scratch + mlp::sc_dt1(M), W, W, saved + mlp::sv_et(M), mlp::kTPad, mlp::kTCh, grads[0], mlp::kTCh, grads[1]);  // time net 1
    g.ndesc = nd;
    block = mlp::wg_place(g);
    hipLaunchKernelGGL(mlp::mlp_wgrad_kernel, dim3(block), dim3(mlp::kWgThreads), 0, s, g);
    return launched("dgs_mlp_backward", -2);
}

// ---- densification statistics ----------------------------------------------------------------------------------------
int dgs_densify_view(int P, const int* radii, const float* g_means2D, float* grad_norm, float* visible, int* radii_vis, void* stream)
{
    if (P < 0 || (P > 0 && (!radii || !g_means2D || !grad_norm || !visible || !radii_vis))) return fail(-1, "dgs_densify_view: bad argument");
    if (P == 0) return 0;
    hipLaunchKernelGGL(densify_view_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, radii, g_means2D, grad_norm,
                       visible, radii_vis);
    return launched("densify_view_kernel");
}

int dgs_densify_accumulate_guarded(int P, const float* grad_norm, const float* visible, const int* radii_vis, float* accum, float* denom,
                                   int* max_radii, const int* skip, void* stream)
{
    if (P < 0 || (P > 0 && (!grad_norm || !visible || !radii_vis || !accum || !denom || !max_radii)))
        return fail(-1, "dgs_densify_accumulate: bad argument");
    if (P == 0) return 0;
    hipLaunchKernelGGL(densify_accum_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, grad_norm, visible, radii_vis,
                       accum, denom, max_radii, skip);
    return launched("densify_accum_kernel");
}

int dgs_densify_accumulate(int P, const float* grad_norm, const float* visible, const int* radii_vis, float* accum, float* denom,
                           int* max_radii, void* stream)
{
    return dgs_densify_accumulate_guarded(P, grad_norm, visible, radii_vis, accum, denom, max_radii, nullptr, stream);
}

}  // extern "C"
