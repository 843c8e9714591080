// surfel_kernels.h -- the per-surfel kernels (gfx950): forward preprocess, fused per-surfel backward, frustum mark, and the staging
// of a workgroup's SH rows that the first two share.
// Replaces preprocessCUDA / computeAABB-bwd / preprocessCUDA-bwd / checkFrustum of the reference (forward.cu:166-260,
// backward.cu:533-649, rasterizer_impl.cu:54-66).
#pragma once
#include <hip/hip_runtime.h>

#include "surfel_math.h"

namespace dgs {

constexpr int kSurfelBlock = 64;    // one wave per workgroup: 12.25 KB of LDS for its SH rows -> 13 workgroups per CU = 832 surfels, so that the 782
                                     // surfels per CU of a 200 k cloud are resident in ONE round (256-thread workgroups: 3 per CU = 768, a second round for 14)

struct PreprocessArgs {
    int P, D, M;
    const float* means3D;
    const float* scales;
    const float* rotations;
    const float* opacities;
    const float* shs;
    const float* colors_precomp;
    Camera cam;
    int* radii;             // [P] out
    float4* rec;            // [P*5] out
    uint2* rects;           // [P] out: packed (tight) tile rectangle of every surfel
    int tight;              // 1: exact opacity-aware rectangles (default), 0: the reference's rectangles
    unsigned row_inv;       // ceil(2^32 / (3 M)) (see surfel_bwd_kernel)
};

// The SH rows of a workgroup's surfels (`total` = rows x row floats, contiguous from `src`) -> LDS rows of `stride` floats.
// 16 bytes per lane and load: at degree 3 the 64 rows are 768 float4, i.e. ONE batch of 12 loads per thread, all in flight
// before the first LDS store -- the 4-byte version was four dependent batches of 12 (a 4-byte load keeps the CU's address unit busy as
// long as a 16-byte one), a third of both per-surfel kernels' run time.  The 4-byte path stays for row counts / alignments
// that do not divide.
__device__ __forceinline__ void stage_sh_rows(const float* __restrict__ src, int total, int row, int stride, unsigned row_inv, float* __restrict__ s_sh)
{
    if ((row & 3) == 0 && (reinterpret_cast<size_t>(src) & 15) == 0) {   // (a float4 never straddles two rows: one row / column per load)
        const float4* __restrict__ src4 = reinterpret_cast<const float4*>(src);
        const int nvec = total >> 2;
        for (int v0 = threadIdx.x; v0 < nvec; v0 += 12 * kSurfelBlock) {
            float4 q[12];
#pragma unroll
            for (int i = 0; i < 12; i++) { const int v = v0 + i * kSurfelBlock; q[i] = v < nvec ? src4[v] : make_float4(0.f, 0.f, 0.f, 0.f); }
#pragma unroll
            for (int i = 0; i < 12; i++) {
                const int v = v0 + i * kSurfelBlock;
                if (v < nvec) {
                    const int e = 4 * v, r = (int)__umulhi((unsigned)e, row_inv);
                    float* d = s_sh + (r * stride + (e - r * row));
                    d[0] = q[i].x; d[1] = q[i].y; d[2] = q[i].z; d[3] = q[i].w;
                }
            }
        }
        return;
    }
    // batches of 12 elements per thread: all loads of a batch are in flight before the first LDS store (an
    // element-wise copy loop is a chain of dependent global-load latencies)
    for (int e0 = threadIdx.x; e0 < total; e0 += 12 * kSurfelBlock) {
        float v[12];
#pragma unroll
        for (int i = 0; i < 12; i++) { const int e = e0 + i * kSurfelBlock; v[i] = e < total ? src[e] : 0.f; }
#pragma unroll
        for (int i = 0; i < 12; i++) {
            const int e = e0 + i * kSurfelBlock;
            if (e < total) { const int r = (int)__umulhi((unsigned)e, row_inv); s_sh[r * stride + (e - r * row)] = v[i]; }
        }
    }
}

__global__ void __launch_bounds__(kSurfelBlock) preprocess_fwd_kernel(PreprocessArgs a)
{
    // SH rows reach the threads through LDS with coalesced loads (see surfel_bwd_kernel)
    extern __shared__ float s_sh[];
    const int base = blockIdx.x * kSurfelBlock;
    const int idx = base + threadIdx.x;
    const int row = a.M * 3, stride = row + 1;
    const bool use_sh = !a.colors_precomp && a.shs;
    // the surfel's own parameters are requested in front of the staging (one memory round trip for both instead of two)
    const int li = min(idx, a.P - 1);
    float pos[3] = {a.means3D[3 * li], a.means3D[3 * li + 1], a.means3D[3 * li + 2]};
    float sc[2] = {a.scales[2 * li], a.scales[2 * li + 1]};
    const float4 qv = reinterpret_cast<const float4*>(a.rotations)[li];
    const float opac = a.opacities[li];
    if (use_sh) {
        const int rows_here = min(kSurfelBlock, a.P - base);
        stage_sh_rows(a.shs + (size_t)base * row, rows_here * row, row, stride, a.row_inv, s_sh);
        __syncthreads();
    }
    if (idx >= a.P) return;
    SurfelRec rec;
    float q[4] = {qv.x, qv.y, qv.z, qv.w};
    const float* sh = use_sh ? s_sh + threadIdx.x * stride : nullptr;
    const float* cp = a.colors_precomp ? a.colors_precomp + 3 * idx : nullptr;
    TileRect tr;
    int tiles;
    const int radius = preprocess_surfel(a.cam, pos, sc, q, opac, a.D, sh, cp, rec, tiles, tr, a.tight != 0);
    a.radii[idx] = radius;
    a.rects[idx] = make_uint2(tr.xs, tr.ys);
    if (radius > 0) {
        const float4* src = reinterpret_cast<const float4*>(&rec);
        float4* dst = a.rec + (size_t)idx * kRecQuads;
#pragma unroll
        for (int c = 0; c < kRecQuads; c++) dst[c] = src[c];
    }
}

struct SurfelBwdArgs {
    int P, D, M;
    const float* means3D;
    const float* scales;
    const float* rotations;
    const float* shs;            // null when colours were precomputed
    unsigned row_inv;            // ceil(2^32 / (3 M)): e / (3 M) == __umulhi(e, row_inv) for the element counts of one workgroup
    Camera cam;
    const int* radii;
    const float4* rec;
    const float* acc;            // [P, kAccFloats] accumulated by the backward blend
    float* dL_dmean2D;           // [P,3]
    float* dL_dnormal;           // [P,3]
    float* dL_dopacity;          // [P]
    float* dL_dcolor;            // [P,3]
    float* dL_dmean3D;           // [P,3]
    float* dL_dtransMat;         // [P,9]
    float* dL_dsh;               // [P,M,3]
    int sh_all_rows;             // 1: dL_dsh is written for EVERY row and coefficient (zeros where the reference leaves the caller's values)
    float* dL_dscale;            // [P,2]
    float* dL_drot;              // [P,4]
};

// Fused computeAABB-bwd + preprocessCUDA-bwd (backward.cu:533-649).  The reference's outputs are caller-zeroed
// (rasterize_points.cu:194-202) and culled surfels left untouched; here the eight per-surfel arrays are written for EVERY row
// (zeros for culled surfels, 112 B each) so that the caller needs no 22 MB fill in front of the backward; dL_dsh keeps the
// reference's rule (visible rows, first (D+1)^2 coefficients): it is the array callers accumulate into (gradient sinks).
__global__ void __launch_bounds__(kSurfelBlock) surfel_bwd_kernel(SurfelBwdArgs a)   // 135 VGPRs; forcing 128 (full residency, 3 spills) measured 43 against 41 us: bandwidth-bound
{
    // SH rows (192 B per surfel at degree 3) are the bulk of this kernel's traffic and one-thread-per-surfel access to
    // them is a 64-way scatter per instruction: the workgroup's rows are staged through LDS with coalesced transfers in
    // both directions (coefficients in, dL_dsh out through the same rows); row stride M*3 + 1 keeps the per-thread row
    // accesses bank-conflict free.
    extern __shared__ float s_sh[];
    const int base = blockIdx.x * kSurfelBlock;
    const int idx = base + threadIdx.x;
    const bool active = idx < a.P && a.radii[idx] > 0;
    const int row = a.M * 3, stride = row + 1;
    const int rows_here = min(kSurfelBlock, a.P - base);
    if (a.shs) {
        stage_sh_rows(a.shs + (size_t)base * row, rows_here * row, row, stride, a.row_inv, s_sh);
        __syncthreads();
    }
    if (active) {
        // (requesting these in front of the staging saves a memory round trip but costs the third wave per SIMD: 191 registers)
        SurfelRec rec;
        {
            float4* dst = reinterpret_cast<float4*>(&rec);
            const float4* src = a.rec + (size_t)idx * kRecQuads;
#pragma unroll
            for (int c = 0; c < kRecQuads; c++) dst[c] = src[c];
        }
        float acc[kAccFloats];
        {
            const float4* src = reinterpret_cast<const float4*>(a.acc + (size_t)idx * kAccFloats);
#pragma unroll
            for (int c = 0; c < kAccFloats / 4; c++) {
                float4 v = src[c];
                acc[4 * c] = v.x; acc[4 * c + 1] = v.y; acc[4 * c + 2] = v.z; acc[4 * c + 3] = v.w;
            }
        }
        float pos[3] = {a.means3D[3 * idx], a.means3D[3 * idx + 1], a.means3D[3 * idx + 2]};
        float sc[2] = {a.scales[2 * idx], a.scales[2 * idx + 1]};
        const float4 qv = reinterpret_cast<const float4*>(a.rotations)[idx];
        float q[4] = {qv.x, qv.y, qv.z, qv.w};
        SurfelGrads g;
        surfel_backward(a.cam, pos, sc, q, rec, acc, g);
        if (a.shs) {
            // coefficients to registers first: sh_backward overwrites the LDS row with dL_dsh while it still reads sh
            float* my = s_sh + threadIdx.x * stride;
            float shr[48];
#pragma unroll
            for (int c = 0; c < 48; c++) shr[c] = c < row ? my[c] : 0.f;
            sh_backward(a.D, shr, pos, a.cam.campos, rec.flags, acc + kAccColor, my, g.dmean3D);
        }
        for (int c = 0; c < 3; c++) {
            a.dL_dmean3D[3 * idx + c] = g.dmean3D[c];
            if (a.dL_dcolor) a.dL_dcolor[3 * idx + c] = acc[kAccColor + c];      // (optional outputs: dgs_surfel_rasterizer.h)
            if (a.dL_dnormal) a.dL_dnormal[3 * idx + c] = acc[kAccNormal + c];
        }
        a.dL_dmean2D[3 * idx] = g.dmean2D[0];
        a.dL_dmean2D[3 * idx + 1] = g.dmean2D[1];
        a.dL_dmean2D[3 * idx + 2] = 0.f;
        a.dL_dopacity[idx] = acc[kAccOpacity];
        if (a.dL_dtransMat)
            for (int c = 0; c < 9; c++) a.dL_dtransMat[9 * idx + c] = g.dT[c];
        a.dL_dscale[2 * idx] = g.dscale[0];
        a.dL_dscale[2 * idx + 1] = g.dscale[1];
        reinterpret_cast<float4*>(a.dL_drot)[idx] = make_float4(g.drot[0], g.drot[1], g.drot[2], g.drot[3]);
    } else if (idx < a.P) {
        for (int c = 0; c < 3; c++) {
            a.dL_dmean3D[3 * idx + c] = 0.f;
            if (a.dL_dcolor) a.dL_dcolor[3 * idx + c] = 0.f;
            if (a.dL_dnormal) a.dL_dnormal[3 * idx + c] = 0.f;
            a.dL_dmean2D[3 * idx + c] = 0.f;
        }
        a.dL_dopacity[idx] = 0.f;
        if (a.dL_dtransMat)
            for (int c = 0; c < 9; c++) a.dL_dtransMat[9 * idx + c] = 0.f;
        a.dL_dscale[2 * idx] = 0.f;
        a.dL_dscale[2 * idx + 1] = 0.f;
        reinterpret_cast<float4*>(a.dL_drot)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (a.shs) {
        // only visible surfels and only the first (D+1)^2 coefficients are written, as in the reference
        __syncthreads();
        static_assert(kSurfelBlock == 64, "one wave per workgroup: the vote below is the workgroup's visibility mask");
        const unsigned long long vis = __ballot(active);   // (was one radii load per element of the loop below)
        const int touched = 3 * (a.D + 1) * (a.D + 1);
        float* dst = a.dL_dsh + (size_t)base * row;
        const int total = rows_here * row;
        if (a.sh_all_rows && (row & 3) == 0 && (reinterpret_cast<size_t>(dst) & 15) == 0) {
            // option 8 (every element is stored: the caller's buffer needs no fill -- a gradient bucket that is stored, not added to):
            // 16 bytes per lane and store
            float4* dst4 = reinterpret_cast<float4*>(dst);
            for (int v = threadIdx.x; v < (total >> 2); v += kSurfelBlock) {
                const int e = 4 * v, r = (int)__umulhi((unsigned)e, a.row_inv), c = e - r * row;
                const float* sp = s_sh + (r * stride + c);
                const bool rv = (vis >> r) & 1ull;
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; k++) o[k] = (rv && c + k < touched) ? sp[k] : 0.f;
                dst4[v] = make_float4(o[0], o[1], o[2], o[3]);
            }
        } else {
            for (int e = threadIdx.x; e < total; e += kSurfelBlock) {
                const int r = (int)__umulhi((unsigned)e, a.row_inv);
                const int c = e - r * row;
                const bool live = c < touched && ((vis >> r) & 1ull);
                if (live) dst[e] = s_sh[r * stride + c];
                else if (a.sh_all_rows) dst[e] = 0.f;   // option 8
            }
        }
    }
}

// checkFrustum (rasterizer_impl.cu:54-66): present = view.z > 0.2
__global__ void __launch_bounds__(256) mark_visible_kernel(int P, const float* means3D, const float* vm, unsigned char* present)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float z = vm[2] * means3D[3 * i] + vm[6] * means3D[3 * i + 1] + vm[10] * means3D[3 * i + 2] + vm[14];
    present[i] = !(z <= 0.2f);
}

}  // namespace dgs
