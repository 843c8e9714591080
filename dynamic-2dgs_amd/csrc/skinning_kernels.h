// skinning_kernels.h -- control-node blend skinning of the surfels (train_ops.hip): every surfel is deformed by its K = 3
// nearest control nodes (utils/time_utils.py of the reference).
//   lbs_fwd_kernel: one thread per surfel; <ASM> also applies the activations render() puts around the deformation.
//   lbs_bwd_kernel: per-node gradient sums, either per-workgroup tables in LDS with bucketed delivery (lbs_deliver) or, for
//     surfels stored by nearest node (COH), wave-level sums and one global table, optionally in 64-bit fixed point (FIXED).
//   lbs_reduce_kernel / lbs_reduce_raw_kernel: the tables -> gradients of the node table / of the raw node parameters.
// lbs_args_table / lbs_args_raw / asm_surfel_args fill the kernels' argument structs for the C entry points.
#pragma once
#include <hip/hip_runtime.h>

#include "wave_reduce.h"

namespace {

// ---- control-node LBS -------------------------------------------------------------------------------------------
constexpr int kLbsK = 3;
constexpr int kLbsHmax = 13;
constexpr int kLbsAttr = 13;       // quaternion 4 | trans 3 | rot 4 | scale 2
constexpr int kLbsBlocks = 256;    // backward: one partial gradient table per workgroup

struct LbsArgs {
    int N, M, H, fstride;
    const float* x; const float* feature; const long long* idx; const float* ntab; const float* attrs; const float* mask;
    // node table rows are tstride floats apart.  rad_raw / w_raw non-null: the table holds only [xyz | hyper] and the
    // kernel radius / weight are exp(rad_raw[j]) / sigmoid(w_raw[j]) (ControlNodeWarp.node_radius / node_weight)
    int tstride; const float* rad_raw; const float* w_raw;
};

// node table rows [xyz | hyper | radius | weight] (dgs_lbs_*)
inline LbsArgs lbs_args_table(int N, int M, int H, const float* x, const float* feature, int fstride, const long long* idx, const float* ntab,
                              const float* attrs, const float* mask)
{
    return LbsArgs{N, M, H, fstride, x, feature, idx, ntab, attrs, mask, 3 + H + 2, nullptr, nullptr};
}
// node rows [xyz | hyper], radius and weight from their raw parameters (dgs_deform_*)
inline LbsArgs lbs_args_raw(int N, int M, int H, const float* x, const float* feature, int fstride, const long long* idx, const float* nodes,
                            const float* rad_raw, const float* w_raw, const float* attrs, const float* mask)
{
    return LbsArgs{N, M, H, fstride, x, feature, idx, nodes, attrs, mask, 3 + H, rad_raw, w_raw};
}

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// activations of the surfel parameters that render() applies around the deformation
// (gaussian_renderer/__init__.py:60-75: means3D = xyz + d_xyz, scales = exp(_scaling) + d_scaling,
//  rotations = normalize(_rotation + d_rotation), opacity = sigmoid(_opacity); scene/gaussian_model.py:60-78)
struct AsmArgs {
    const float* scaling_raw; const float* rotation_raw; const float* opacity_raw;
    float* means3D; float* scales; float* rotations; float* opacity;                                   // forward out
    const float* g_means3D; const float* g_scales; const float* g_rotations; const float* g_opacity;   // backward in
    float* g_xyz; float* g_scaling_raw; float* g_rotation_raw; float* g_opacity_raw;                   // backward out
};

// the raw surfel parameters both directions read; the caller adds its outputs (forward) or gradients (backward)
inline AsmArgs asm_surfel_args(const float* scaling_raw, const float* rotation_raw, const float* opacity_raw)
{
    AsmArgs s{};
    s.scaling_raw = scaling_raw; s.rotation_raw = rotation_raw; s.opacity_raw = opacity_raw;
    return s;
}

// quaternion (r,i,j,k), not necessarily unit -> rotation matrix, utils/time_utils.py:115-132
__device__ __forceinline__ void quat_to_mat(const float* q, float* R, float& two_s)
{
    const float r = q[0], i = q[1], j = q[2], k = q[3];
    two_s = 2.0f / (r * r + i * i + j * j + k * k);
    R[0] = 1 - two_s * (j * j + k * k); R[1] = two_s * (i * j - k * r); R[2] = two_s * (i * k + j * r);
    R[3] = two_s * (i * j + k * r); R[4] = 1 - two_s * (i * i + k * k); R[5] = two_s * (j * k - i * r);
    R[6] = two_s * (i * k - j * r); R[7] = two_s * (j * k + i * r); R[8] = 1 - two_s * (i * i + j * j);
}

// Table rows are gathered per lane (every lane another row): 4-byte aligned 16-byte loads fetch a row in 3-4 instructions
// instead of 11-13 scalar ones; the texture path spends its time per instruction and per cache line touched, not per byte.
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void load_row(const float* __restrict__ src, int n, float* __restrict__ out /*[16]*/)
{
#pragma unroll
    for (int c = 0; c < 16; c += 4) {
        if (c + 4 <= n) {
            const f4u v = *reinterpret_cast<const f4u*>(src + c);
            out[c] = v.x; out[c + 1] = v.y; out[c + 2] = v.z; out[c + 3] = v.w;
        } else {
#pragma unroll
            for (int d = c; d < c + 4; d++) out[d] = d < n ? src[d] : 0.f;
        }
    }
}

// per-point evaluation shared by forward and backward
struct LbsPoint {
    float w[kLbsK], e[kLbsK], dist[kLbsK], Ax[kLbsK][3], rad[kLbsK], wg[kLbsK];
    float W;
    int j[kLbsK];
};

template <int HM = kLbsHmax>
__device__ __forceinline__ void lbs_eval(const LbsArgs& a, int n, LbsPoint& p, float* xq /*[3+HM]*/)
{
    const int T = a.tstride;
    xq[0] = a.x[3 * n]; xq[1] = a.x[3 * n + 1]; xq[2] = a.x[3 * n + 2];
    {
        float fr[16];
        load_row(a.feature + (size_t)n * a.fstride, a.H < 16 ? a.H : 16, fr);
        for (int h = 0; h < HM; h++) xq[3 + h] = fr[h];
    }
    p.W = 0.f;
#pragma unroll
    for (int k = 0; k < kLbsK; k++) {
        const int j = (int)a.idx[(size_t)n * kLbsK + k];
        p.j[k] = j;
        float nd[16], at[16];
        load_row(a.ntab + (size_t)j * T, T < 16 ? T : 16, nd);
        load_row(a.attrs + (size_t)j * kLbsAttr, kLbsAttr, at);
        float dist = 0.f;
        for (int c = 0; c < 3 + HM; c++)
            if (c < 3 + a.H) { const float t = xq[c] - nd[c]; dist += t * t; }
        const float r = a.rad_raw ? expf(a.rad_raw[j]) : a.ntab[(size_t)j * T + 3 + a.H];
        const float wg = a.w_raw ? sigmoidf_(a.w_raw[j]) : a.ntab[(size_t)j * T + 3 + a.H + 1];
        p.rad[k] = r; p.wg[k] = wg;
        p.dist[k] = dist;
        p.e[k] = expf(-dist / (2.f * r * r));
        p.w[k] = p.e[k] * wg + 1e-7f;
        p.W += p.w[k];
        float R[9], two_s;
        quat_to_mat(at, R, two_s);
        const float dx = xq[0] - nd[0], dy = xq[1] - nd[1], dz = xq[2] - nd[2];
        p.Ax[k][0] = R[0] * dx + R[1] * dy + R[2] * dz + nd[0] + at[4];
        p.Ax[k][1] = R[3] * dx + R[4] * dy + R[5] * dz + nd[1] + at[5];
        p.Ax[k][2] = R[6] * dx + R[7] * dy + R[8] * dz + nd[2] + at[6];
    }
}

template <bool ASM>
__global__ void __launch_bounds__(256) lbs_fwd_kernel(LbsArgs a, float* d_xyz, float* d_rot, float* d_scale, AsmArgs s_)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= a.N) return;
    LbsPoint p;
    float xq[3 + kLbsHmax];
    lbs_eval(a, n, p, xq);
    const float inv = 1.0f / p.W, m = a.mask ? a.mask[n] : 1.0f;
    float t[3] = {0, 0, 0}, q[4] = {0, 0, 0, 0}, s[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < kLbsK; k++) {
        const float w = p.w[k] * inv;
        float at[16];
        load_row(a.attrs + (size_t)p.j[k] * kLbsAttr, kLbsAttr, at);
        for (int c = 0; c < 3; c++) t[c] += w * p.Ax[k][c];
        for (int c = 0; c < 4; c++) q[c] += w * at[7 + c];
        for (int c = 0; c < 2; c++) s[c] += w * at[11 + c];
    }
    if (!ASM) {
        for (int c = 0; c < 3; c++) d_xyz[3 * n + c] = (t[c] - xq[c]) * m;
        for (int c = 0; c < 4; c++) d_rot[4 * n + c] = q[c] * m;
        for (int c = 0; c < 2; c++) d_scale[2 * n + c] = s[c] * m;
    } else {
        for (int c = 0; c < 3; c++) s_.means3D[3 * n + c] = xq[c] + (t[c] - xq[c]) * m;
        for (int c = 0; c < 2; c++) s_.scales[2 * n + c] = expf(s_.scaling_raw[2 * n + c]) + s[c] * m;
        float v[4], n2 = 0.f;
        for (int c = 0; c < 4; c++) { v[c] = s_.rotation_raw[4 * n + c] + q[c] * m; n2 += v[c] * v[c]; }
        const float invn = 1.0f / fmaxf(sqrtf(n2), 1e-12f);   // F.normalize
        for (int c = 0; c < 4; c++) s_.rotations[4 * n + c] = v[c] * invn;
        s_.opacity[n] = sigmoidf_(s_.opacity_raw[n]);
    }
}

// Backward.  Per-node gradients (13 attribute + H+2 table columns) of the ~782 points of a workgroup are accumulated
// in an LDS table with ds_add_f32 and written once as that workgroup's partial table; lbs_reduce_kernel sums the
// kLbsBlocks partials.  (Direct global atomics would be ~7 M adds onto ~24 k hot addresses.)
constexpr int kLbsBwdThreads = 512;    // one workgroup per CU (the LDS table is ~94 KB); 8 waves keep 256 VGPRs per lane (no spills)

// LDS float atomics are the wrong tool here: ds_add_f32 retires ~1 lane per 2.4 clocks on gfx950 (measured: 13.8 M lane
// adds = 55 of this kernel's 104 us; the same pattern with ds_add_u32 takes 8 us, tools/micro/lds_atomic_bench.hip; the
// bucketed delivery below costs ~40 us, LDS-instruction bound, and makes the sums deterministic).
// The per-node sums are therefore built without float atomics: for each of the K neighbour slots the workgroup's threads
// park their G contributions in an LDS exchange buffer and take a slot in the target node's small bucket with an integer
// atomic (fast); after one barrier the thread that OWNS a node adds the parked rows into the node's table row with plain
// read-modify-writes.  Buckets hold kLbsSlots rows; the rare excess is added with float atomics in a second, guarded phase.
constexpr int kLbsSlots = 4;   // parked rows per node and delivery round; the rare excess goes through float atomics afterwards

__device__ __forceinline__ void lbs_deliver(bool valid, int j, const float* cv, int G, int GS, int M, float* s_tab, float* s_exch,
                                            int* s_cnt, unsigned short* s_slot, int* s_over)
{
    // on entry: s_cnt[] == 0, *s_over == 0 (left that way by the previous round)
    const int tid = threadIdx.x;
    int pos = 0;
    if (valid) {
        pos = atomicAdd(&s_cnt[j], 1);                       // integer LDS atomic: fast
        if (pos < kLbsSlots) {
            s_slot[j * kLbsSlots + pos] = (unsigned short)tid;
#pragma unroll
            for (int c = 0; c < kLbsAttr + kLbsHmax + 2; c++)
                if (c < G) s_exch[tid * GS + c] = cv[c];
        } else {
            *s_over = 1;
        }
    }
    __syncthreads();
    for (int node = tid; node < M; node += kLbsBwdThreads) {
        const int cn = min(s_cnt[node], kLbsSlots);
        if (cn == 0) continue;
        s_cnt[node] = 0;
        float* row = s_tab + (size_t)node * G;
        // all reads of a row are independent (static unroll): one LDS latency per row instead of one per element
        float accv[kLbsAttr + kLbsHmax + 2];
#pragma unroll
        for (int c = 0; c < kLbsAttr + kLbsHmax + 2; c++) accv[c] = c < G ? row[c] : 0.f;
        for (int e = 0; e < cn; e++) {
            const float* src = s_exch + (int)s_slot[node * kLbsSlots + e] * GS;
#pragma unroll
            for (int c = 0; c < kLbsAttr + kLbsHmax + 2; c++) accv[c] += c < G ? src[c] : 0.f;
        }
#pragma unroll
        for (int c = 0; c < kLbsAttr + kLbsHmax + 2; c++)
            if (c < G) row[c] = accv[c];
    }
    __syncthreads();
    if (*s_over) {   // workgroup-uniform; ~1 round in 6 on the metric scene has a node with more than kLbsSlots rows
        if (valid && pos >= kLbsSlots) {
            float* row = s_tab + (size_t)j * G;
#pragma unroll
            for (int c = 0; c < kLbsAttr + kLbsHmax + 2; c++)
                if (c < G) atomicAdd(row + c, cv[c]);
        }
        __syncthreads();
        if (tid == 0) *s_over = 0;
        // the owners above zero only the counters they served; counters of overfull nodes were zeroed too (cn > 0)
        __syncthreads();
    }
}

__host__ __device__ inline int lbs_exch_stride(int G) { return G | 1; }   // odd row stride: conflict-free row writes
inline size_t lbs_bwd_lds_bytes(int M, int H)
{
    const int G = kLbsAttr + H + 2;
    return ((size_t)M * G + (size_t)kLbsBwdThreads * lbs_exch_stride(G)) * sizeof(float) + (size_t)M * sizeof(int) +
           (size_t)M * kLbsSlots * sizeof(unsigned short) + 16;
}

// Coherent variant (COH): for surfels STORED IN THE ORDER OF THEIR NEAREST CONTROL NODE (Trainer.sort_surfels) the 64 points
// of a wave share one or two nodes in the first neighbour slot and ~10 in the others.  The wave sums each node's
// contributions across its lanes (wave_reduce.h: permlane swaps + DPP, no LDS) and issues ONE 23-lane global atomic per
// (wave, node) into a single [M][G] table -- no per-workgroup tables (24 MB of partials to write and re-read), no LDS, 782
// small workgroups instead of 256 large ones.  Measured at 200 k surfels / 1024 nodes: 97 + 15 us (LDS tables + reduction of
// the partials) -> 77 + 5 us; the kernel is memory-latency bound either way (3 waves per SIMD in total, PMC: 62 % of the
// wave cycles parked on s_waitcnt); a variant that first combined the waves of a 512-thread workgroup in an LDS hash table
// (4x fewer global atomics) measured 96 us, issuing every atomic of a point after its last load / store 78 us.
// What it waits for is RESIDENCY: 200 k surfels are 3125 waves, 153 VGPRs allow 3 waves per SIMD = 3072 -- the last 53 waves
// (14 workgroups) run in a second round and the kernel takes two wave lifetimes.  Forcing 128 VGPRs spilled 68 registers
// (82 us); specialising the kernel for the trainer's hyper dimension (template HT = 8: arrays sized for it, static indices)
// needs 127 without a spill: all waves resident in one round, 77 -> 53 us.
// Correct for any order; an unsorted cloud makes the loop below run once per DISTINCT node of a wave (up to 64 times).
constexpr int kCohThreads = 256;

// FIXED (dgs_deform_backward accumulate bit 4): the table holds 64-bit fixed-point sums (units of 2^-44) added with INTEGER
// atomics -- order-free, so the node gradients are bit-identical from run to run (Trainer.set_deterministic); the reduce converts.
__device__ __forceinline__ unsigned long long lbs_to_fixed44(float v)
{
    v = fminf(fmaxf(v, -262144.0f), 262144.0f);
    return (unsigned long long)__float2ll_rn(v * 17592186044416.0f);
}
__device__ __forceinline__ float lbs_from_fixed44(unsigned long long v) { return (float)((double)(long long)v * (1.0 / 17592186044416.0)); }

template <bool FIXED, int CVN>
__device__ __forceinline__ void lbs_combine(bool valid, int j, const float (&cv)[CVN], int G, float* __restrict__ table)
{
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(valid);
    while (todo != 0ull) {
        const int jl = __builtin_amdgcn_readlane(j, __builtin_ctzll(todo));   // wave-uniform node id
        const bool sel = valid && j == jl;
        // columns 0..15, then 16..23 (G <= 24 here: 13 attributes + H <= 9 + 2; wider tables take the generic path below)
        float r0, r1 = 0.f, r2 = 0.f;
        {
            float lo[16];
#pragma unroll
            for (int c = 0; c < 16; c++) lo[c] = (sel && c < G && c < CVN) ? cv[c < CVN ? c : 0] : 0.f;
            r0 = dgs::wave_reduce16_dpp(lo);   // quad q holds the wave total of column q
        }
        {
            float hi[8];
#pragma unroll
            for (int c = 0; c < 8; c++) hi[c] = (sel && 16 + c < G && 16 + c < CVN) ? cv[16 + c < CVN ? 16 + c : 0] : 0.f;
            r1 = dgs::wave_reduce8_dpp(hi);    // lanes 8 k .. 8 k + 7 hold the total of column 16 + k
        }
        if (CVN > 24 && G > 24) {              // hyper_dim > 9: four more columns (wave-uniform, never taken by the trainer)
            float hi[8];
#pragma unroll
            for (int c = 0; c < 8; c++) hi[c] = (sel && 24 + c < G && 24 + c < CVN) ? cv[24 + c < CVN ? 24 + c : 0] : 0.f;
            r2 = dgs::wave_reduce8_dpp(hi);
        }
        const int sub4 = lane & 3, sub8 = lane & 7;
        const int col = sub4 == 0 ? (lane >> 2) : (sub8 == 1 ? 16 + (lane >> 3) : (sub8 == 2 ? 24 + (lane >> 3) : -1));
        if (col >= 0 && col < G) {
            const float tot = sub4 == 0 ? r0 : (sub8 == 1 ? r1 : r2);
            if (FIXED) atomicAdd(reinterpret_cast<unsigned long long*>(table) + (size_t)jl * G + col, lbs_to_fixed44(tot));
            else atomicAdd(table + (size_t)jl * G + col, tot);
        }
        todo &= ~__ballot(sel);
    }
}

// HT > 0: hyper dimension known at compile time (a.H == HT): arrays sized for it, static indexing (the trainer's H = 8)
template <bool ASM, bool COH, int HT = 0, bool FIXED = false>
__global__ void __launch_bounds__(COH ? kCohThreads : kLbsBwdThreads) lbs_bwd_kernel(LbsArgs a, const float* g_xyz, const float* g_rot, const float* g_scale,
                                                      float* g_feature, int gf_stride, int accumulate,
                                                      float* partial /*[kLbsBlocks][M][G], COH: [M][G] zeroed*/, int chunk, AsmArgs s_)
{
    extern __shared__ float s_tab[];  // [M][G], G = 13 + H + 2, then the exchange buffer and the integer arrays of lbs_deliver
    constexpr int HM = HT > 0 ? HT : kLbsHmax;
    const int H = HT > 0 ? HT : a.H;
    const int G = kLbsAttr + H + 2, GS = lbs_exch_stride(G);
    const int T = a.tstride;
    float* s_exch = s_tab + (size_t)a.M * G;
    int* s_cnt = reinterpret_cast<int*>(s_exch + (size_t)kLbsBwdThreads * GS);
    int* s_over = s_cnt + a.M;
    unsigned short* s_slot = reinterpret_cast<unsigned short*>(s_over + 2);
    constexpr int kThreads = COH ? kCohThreads : kLbsBwdThreads;
    if (!COH) {
        for (int i = threadIdx.x; i < a.M * G; i += kLbsBwdThreads) s_tab[i] = 0.f;
        for (int i = threadIdx.x; i < a.M; i += kLbsBwdThreads) s_cnt[i] = 0;
        if (threadIdx.x == 0) *s_over = 0;
        __syncthreads();
    }
    const int begin = blockIdx.x * chunk, end = min(a.N, (int)(blockIdx.x + 1) * chunk);
    for (int n0 = begin; n0 < end; n0 += kThreads) {   // uniform trip count: lbs_deliver synchronises the workgroup
        const int n = n0 + threadIdx.x;
        const bool valid = n < end;
        LbsPoint p;
        float xq[3 + HM];
        float gx[3] = {0, 0, 0}, gq[4] = {0, 0, 0, 0}, gs[2] = {0, 0};
        float inv = 0.f, m = 0.f;
        if (valid) {
            lbs_eval<HM>(a, n, p, xq);
            inv = 1.0f / p.W;
            m = a.mask ? a.mask[n] : 1.0f;
        if (!ASM) {
            for (int c = 0; c < 3; c++) gx[c] = g_xyz[3 * n + c] * m;
            for (int c = 0; c < 4; c++) gq[c] = g_rot[4 * n + c] * m;
            for (int c = 0; c < 2; c++) gs[c] = g_scale[2 * n + c] * m;
        } else {
            // adjoint of the activations (see AsmArgs); the deformation sees the detached centre, so the centre's own
            // gradient is just the incoming one
            for (int c = 0; c < 3; c++) {
                const float g = s_.g_means3D[3 * n + c];
                gx[c] = g * m;
                s_.g_xyz[3 * n + c] = accumulate ? s_.g_xyz[3 * n + c] + g : g;
            }
            for (int c = 0; c < 2; c++) {
                const float g = s_.g_scales[2 * n + c];
                gs[c] = g * m;
                const float v = g * expf(s_.scaling_raw[2 * n + c]);
                s_.g_scaling_raw[2 * n + c] = accumulate ? s_.g_scaling_raw[2 * n + c] + v : v;
            }
            float q[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < kLbsK; k++) {
                const f4u r4 = *reinterpret_cast<const f4u*>(a.attrs + (size_t)p.j[k] * kLbsAttr + 7);
                const float wn = p.w[k] * inv;
                q[0] += wn * r4.x; q[1] += wn * r4.y; q[2] += wn * r4.z; q[3] += wn * r4.w;
            }
            float v[4], n2 = 0.f, dot = 0.f;
            for (int c = 0; c < 4; c++) { v[c] = s_.rotation_raw[4 * n + c] + q[c] * m; n2 += v[c] * v[c]; }
            const float nrm = sqrtf(n2);
            const bool tiny = nrm < 1e-12f;
            const float invn = 1.0f / fmaxf(nrm, 1e-12f);
            for (int c = 0; c < 4; c++) dot += v[c] * invn * s_.g_rotations[4 * n + c];
            for (int c = 0; c < 4; c++) {
                const float g = tiny ? s_.g_rotations[4 * n + c] * invn : (s_.g_rotations[4 * n + c] - v[c] * invn * dot) * invn;
                gq[c] = g * m;
                s_.g_rotation_raw[4 * n + c] = accumulate ? s_.g_rotation_raw[4 * n + c] + g : g;
            }
            const float o = sigmoidf_(s_.opacity_raw[n]);
            const float go = s_.g_opacity[n] * o * (1.0f - o);
            s_.g_opacity_raw[n] = accumulate ? s_.g_opacity_raw[n] + go : go;
        }
        }
        float dwh[kLbsK] = {0, 0, 0}, mean = 0.f;  // d loss / d (normalised weight)
        if (valid) {
#pragma unroll
        for (int k = 0; k < kLbsK; k++) {
            float at[16];
            load_row(a.attrs + (size_t)p.j[k] * kLbsAttr, kLbsAttr, at);
            float v = p.Ax[k][0] * gx[0] + p.Ax[k][1] * gx[1] + p.Ax[k][2] * gx[2];
            for (int c = 0; c < 4; c++) v += at[7 + c] * gq[c];
            for (int c = 0; c < 2; c++) v += at[11 + c] * gs[c];
            dwh[k] = v;
            mean += p.w[k] * inv * v;
        }
        }
        float gfeat[HM];
        for (int h = 0; h < HM; h++) gfeat[h] = 0.f;
#pragma unroll
        for (int k = 0; k < kLbsK; k++) {
            float cv[kLbsAttr + HM + 2];   // this point's contribution to node p.j[k]: [attrs 13 | hyper H | radius | weight]
            int j = 0;
            if (valid) {
            j = p.j[k];
            const float wn = p.w[k] * inv;
            float nd[16], at[16];
            load_row(a.ntab + (size_t)j * T, T < 16 ? T : 16, nd);
            load_row(a.attrs + (size_t)j * kLbsAttr, 4, at);   // only the local-frame quaternion is needed here
            // ---- attributes: rotation quaternion through R, translation, rotation/scale residuals
            const float dA[3] = {wn * gx[0], wn * gx[1], wn * gx[2]};
            const float dl[3] = {xq[0] - nd[0], xq[1] - nd[1], xq[2] - nd[2]};
            float Gm[9];
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Gm[3 * r + c] = dA[r] * dl[c];
            {
                const float r = at[0], i = at[1], jq = at[2], kq = at[3];
                const float n2 = r * r + i * i + jq * jq + kq * kq, two_s = 2.0f / n2;
                const float B[9] = {-(jq * jq + kq * kq), i * jq - kq * r, i * kq + jq * r, i * jq + kq * r, -(i * i + kq * kq),
                                    jq * kq - i * r, i * kq - jq * r, jq * kq + i * r, -(i * i + jq * jq)};
                float BG = 0.f;
                for (int c = 0; c < 9; c++) BG += B[c] * Gm[c];
                const float dBr = -kq * Gm[1] + jq * Gm[2] + kq * Gm[3] - i * Gm[5] - jq * Gm[6] + i * Gm[7];
                const float dBi = jq * (Gm[1] + Gm[3]) + kq * (Gm[2] + Gm[6]) - 2.f * i * (Gm[4] + Gm[8]) + r * (Gm[7] - Gm[5]);
                const float dBj = -2.f * jq * (Gm[0] + Gm[8]) + i * (Gm[1] + Gm[3]) + r * (Gm[2] - Gm[6]) + kq * (Gm[5] + Gm[7]);
                const float dBk = -2.f * kq * (Gm[0] + Gm[4]) + r * (Gm[3] - Gm[1]) + i * (Gm[2] + Gm[6]) + jq * (Gm[5] + Gm[7]);
                const float cs = -4.0f * BG / (n2 * n2);
                cv[0] = two_s * dBr + cs * r;
                cv[1] = two_s * dBi + cs * i;
                cv[2] = two_s * dBj + cs * jq;
                cv[3] = two_s * dBk + cs * kq;
            }
            for (int c = 0; c < 3; c++) cv[4 + c] = dA[c];
            for (int c = 0; c < 4; c++) cv[7 + c] = wn * gq[c];
            for (int c = 0; c < 2; c++) cv[11 + c] = wn * gs[c];
            // ---- weights: w = e * weight + 1e-7, e = exp(-dist / (2 r^2)), normalised over the K neighbours
            const float dw = (dwh[k] - mean) * inv;
            const float rad = p.rad[k], wg = p.wg[k];
            const float de = dw * wg * p.e[k];
            const float ddist = -de / (2.f * rad * rad);
            const float d_rad = de * p.dist[k] / (rad * rad * rad), d_w = dw * p.e[k];
#pragma unroll
            for (int h = 0; h < HM; h++) {
                const float gd = h < H ? 2.f * (xq[3 + h] - nd[3 + h]) * ddist : 0.f;
                gfeat[h] += gd;
                // columns 13 .. 13+H-1: node hyper coordinates, then radius, weight (static register indices only)
                cv[kLbsAttr + h] = h < H ? -gd : (h == H ? d_rad : (h == H + 1 ? d_w : 0.f));
            }
#pragma unroll
            for (int h = HM; h < HM + 2; h++) cv[kLbsAttr + h] = h == H ? d_rad : (h == H + 1 ? d_w : 0.f);
            }
            if (COH) lbs_combine<FIXED>(valid, j, cv, G, partial);
            else lbs_deliver(valid, j, cv, G, GS, a.M, s_tab, s_exch, s_cnt, s_slot, s_over);
        }
        if (valid)
        for (int h = 0; h < HM; h++)
            if (h < H) {
                float* dst = g_feature + (size_t)n * gf_stride + h;
                *dst = accumulate ? *dst + gfeat[h] : gfeat[h];
            }

    }
    if (COH) return;
    __syncthreads();
    float* dst = partial + (size_t)blockIdx.x * a.M * G;
    for (int i = threadIdx.x; i < a.M * G; i += kLbsBwdThreads) dst[i] = s_tab[i];
}

__global__ void __launch_bounds__(256) lbs_reduce_kernel(const float* partial, int M, int H, float* g_ntab, float* g_attrs, int nparts)
{
    const int G = kLbsAttr + H + 2, T = 3 + H + 2;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M * G) return;
    float acc = 0.f;
    for (int b = 0; b < nparts; b++) acc += partial[(size_t)b * M * G + i];
    const int node = i / G, c = i - node * G;
    if (c < kLbsAttr) g_attrs[(size_t)node * kLbsAttr + c] = acc;
    else g_ntab[(size_t)node * T + 3 + (c - kLbsAttr)] = acc;
    if (c < 3) g_ntab[(size_t)node * T + c] = 0.f;  // node positions are detached in the reference
}

// raw-parameter variant: gradients of nodes[M, 3+H] (hyper columns), _node_radius (through exp) and _node_weight
// (through sigmoid), written or added in place; the attribute gradients are always written (the node MLP consumes them)
__global__ void __launch_bounds__(256) lbs_reduce_raw_kernel(const float* partial, int M, int H, const float* rad_raw,
                                                             const float* w_raw, float* g_nodes, float* g_rad_raw, float* g_w_raw,
                                                             float* g_attrs, int accumulate, int nparts, float* clear, int fixed = 0)
{
    const int G = kLbsAttr + H + 2, T = 3 + H;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M * G) return;
    float acc = 0.f;
    if (fixed) {   // one [M][G] table of 64-bit fixed-point sums (lbs_combine<FIXED>)
        unsigned long long* t64 = reinterpret_cast<unsigned long long*>(const_cast<float*>(partial));
        acc = lbs_from_fixed44(t64[i]);
        if (clear) t64[i] = 0ull;
    } else {
    for (int b = 0; b < nparts; b++) acc += partial[(size_t)b * M * G + i];
    if (clear) clear[i] = 0.f;   // coherent variant with a persistent table: leave it zeroed for the next backward (no memset launch)
    }
    const int node = i / G, c = i - node * G;
    if (c < kLbsAttr) { g_attrs[(size_t)node * kLbsAttr + c] = acc; }
    else if (c < kLbsAttr + H) {
        float* d = g_nodes + (size_t)node * T + 3 + (c - kLbsAttr);
        *d = accumulate ? *d + acc : acc;
    } else if (c == kLbsAttr + H) {
        const float v = acc * expf(rad_raw[node]);
        g_rad_raw[node] = accumulate ? g_rad_raw[node] + v : v;
    } else {
        const float w = sigmoidf_(w_raw[node]);
        const float v = acc * w * (1.0f - w);
        g_w_raw[node] = accumulate ? g_w_raw[node] + v : v;
    }
    if (c < 3 && !accumulate) g_nodes[(size_t)node * T + c] = 0.f;
}

}  // namespace
