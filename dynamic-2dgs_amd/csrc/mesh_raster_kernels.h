// mesh_raster_kernels.h -- the z-buffer triangle rasterizer of the mesh images (mesh_ops.hip: dgs_mesh_raster, dgs_mesh_resolve).
#pragma once
#include <hip/hip_runtime.h>

namespace {

// ---- triangle rasterizer --------------------------------------------------------------------------------------------------------
// The arithmetic of one (face, pixel) pair is ras_pair, shared by the three kernels; include/dgs_mesh_ops.h states it.  Per pair:
// 6 subtractions, 9 multiplications (3 of them by the sign), 3 differences, the compares, 2 additions, then -- for covered pixels
// only -- 3 divisions, 3 multiplications, 2 additions, 1 division, one load of best[P] and, if the candidate is nearer, the atomic.
// Small path: a lane owns a face and walks its box (at most RAS_SMALL_AREA pixels): the extracted meshes' faces cover 1 - 4 pixels,
//   so a lane does a handful of tests after one 96-byte row fetch (six 16-byte loads).
// Large path: a workgroup owns a face (or a stripe of its rows when few faces share many workgroups; above 2^22 faces, several
//   faces in turn), its 256 threads form a
//   64 x 4 pixel tile that steps over the box -- a wave touches 64 consecutive pixels of one image row; the row address is
//   uniform, so the compiler fetches it once per wave.
constexpr int RAS_THREADS = 256, RAS_SMALL_AREA = 64, RAS_ROW = 24, RAS_ROW4 = RAS_ROW / 4, RAS_MAX_C = 8, RAS_TILE_X = 64,
              RAS_TILE_Y = RAS_THREADS / RAS_TILE_X, RAS_MAX_STRIPES = 64, RAS_TARGET_GROUPS = 2048, RAS_MAX_GROUPS = 1 << 22;
constexpr unsigned long long RAS_EMPTY = ~0ull;

struct RasFace {
    float xa[3], ya[3], dx[3], dy[3], s[3], sa, iw[3];
    int x0, x1, y0, y1;
};

__device__ __forceinline__ RasFace ras_load(const float4* __restrict__ table, long long face, int H, int W) {
    const float4* row = table + face * RAS_ROW4;
    RasFace f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 e = row[k];
        f.xa[k] = e.x, f.ya[k] = e.y, f.dx[k] = e.z, f.dy[k] = e.w;
    }
    const float4 s = row[3], iw = row[4], b = row[5];
    f.s[0] = s.x, f.s[1] = s.y, f.s[2] = s.z, f.sa = s.w;
    f.iw[0] = iw.x, f.iw[1] = iw.y, f.iw[2] = iw.z;
    // the box is clamped to the image again, whatever the table says: no pixel index below can leave [0, H * W)
    f.x0 = max(__float_as_int(b.x), 0), f.x1 = min(__float_as_int(b.y), W - 1);
    f.y0 = max(__float_as_int(b.z), 0), f.y1 = min(__float_as_int(b.w), H - 1);
    return f;
}

// covered?  b[] and z are only meaningful when it returns true
__device__ __forceinline__ bool ras_pair(const RasFace& f, float px, float py, float b[3], float& z) {
    float e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = f.s[k] * (f.dx[k] * (py - f.ya[k]) - f.dy[k] * (px - f.xa[k]));
    const bool pos = (e[0] >= 0.0f) & (e[1] >= 0.0f) & (e[2] >= 0.0f), neg = (e[0] <= 0.0f) & (e[1] <= 0.0f) & (e[2] <= 0.0f);
    const float S = (e[0] + e[1]) + e[2];
    if (!(((f.sa > 0.0f) & pos) | ((f.sa < 0.0f) & neg)) || !(S != 0.0f)) return false;
    b[0] = e[0] / S, b[1] = e[1] / S, b[2] = e[2] / S;
    const float q = (b[0] * f.iw[0] + b[1] * f.iw[1]) + b[2] * f.iw[2];
    z = 1.0f / q;
    return q > 0.0f;                                                        // not NaN (an edge function that overflowed), so z > 0
}

__device__ __forceinline__ void ras_visit(const RasFace& f, unsigned face, int x, int y, int W, unsigned long long* best) {
    float b[3], z;
    if (!ras_pair(f, (float)x, (float)y, b, z)) return;
    const unsigned long long cand = ((unsigned long long)__float_as_uint(z) << 32) | face;
    unsigned long long* p = best + ((size_t)y * W + x);                     // 0 <= x < W, 0 <= y < H: ras_load clamped the box
    if (cand < *p) atomicMin(p, cand);                                      // a stale read is a larger value: at worst one atomic more
}

__global__ __launch_bounds__(RAS_THREADS) void raster_small_kernel(long long n_faces, const float4* __restrict__ table,
                                                                   const int* __restrict__ list, long long n_list, int H, int W,
                                                                   unsigned long long* best) {
    const long long i = (long long)blockIdx.x * RAS_THREADS + threadIdx.x;
    if (i >= n_list) return;
    const int face = list[i];
    if (face < 0 || face >= n_faces) return;
    const RasFace f = ras_load(table, face, H, W);
    for (int y = f.y0; y <= f.y1; ++y)
        for (int x = f.x0; x <= f.x1; ++x) ras_visit(f, (unsigned)face, x, y, W, best);
}

__global__ __launch_bounds__(RAS_THREADS) void raster_large_kernel(long long n_faces, const float4* __restrict__ table,
                                                                   const int* __restrict__ list, long long n_list, int H, int W,
                                                                   unsigned long long* best) {
    const int tx = threadIdx.x % RAS_TILE_X, ty = threadIdx.x / RAS_TILE_X;
    const int step = RAS_TILE_Y * (int)gridDim.y;                           // <= 4 * 64; y < H <= 2^30: no overflow
    for (long long i = blockIdx.x; i < n_list; i += gridDim.x) {            // gridDim.x = min(n_list, RAS_MAX_GROUPS)
        const int face = list[i];
        if (face < 0 || face >= n_faces) continue;
        const RasFace f = ras_load(table, face, H, W);
        for (int y = f.y0 + RAS_TILE_Y * (int)blockIdx.y + ty; y <= f.y1; y += step)
            for (int x = f.x0 + tx; x <= f.x1; x += RAS_TILE_X) ras_visit(f, (unsigned)face, x, y, W, best);
    }
}

__global__ __launch_bounds__(RAS_THREADS) void raster_resolve_kernel(int H, int W, const unsigned long long* __restrict__ best, long long n_faces,
                                                                     const float4* __restrict__ table, const int* __restrict__ faces,
                                                                     long long n_vertices, const float* __restrict__ attr, int C,
                                                                     const float* __restrict__ background, int* __restrict__ face_id,
                                                                     float* __restrict__ depth, float* __restrict__ bary,
                                                                     float* __restrict__ image) {
    const size_t n = (size_t)H * W, p = (size_t)blockIdx.x * RAS_THREADS + threadIdx.x;
    if (p >= n) return;
    const unsigned long long v = best[p];
    const long long face = (long long)(v & 0xFFFFFFFFull);
    const bool hit = v != RAS_EMPTY && face < n_faces;
    float b[3] = {0.0f, 0.0f, 0.0f}, z = 0.0f, w[3] = {0.0f, 0.0f, 0.0f};
    int corner[3] = {0, 0, 0};
    bool shade = false;
    if (hit) {
        const RasFace f = ras_load(table, face, H, W);
        const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
        float e[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = f.s[k] * (f.dx[k] * ((float)y - f.ya[k]) - f.dy[k] * ((float)x - f.xa[k]));
        const float S = (e[0] + e[1]) + e[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) b[k] = e[k] / S, w[k] = b[k] * f.iw[k];
        z = 1.0f / ((w[0] + w[1]) + w[2]);
        if (C > 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) corner[k] = faces[3 * face + k];
            shade = corner[0] >= 0 && corner[0] < n_vertices && corner[1] >= 0 && corner[1] < n_vertices && corner[2] >= 0 && corner[2] < n_vertices;
        }
    }
    if (face_id) face_id[p] = hit ? (int)face : -1;
    if (depth) depth[p] = z;
    if (bary) bary[3 * p] = b[0], bary[3 * p + 1] = b[1], bary[3 * p + 2] = b[2];
    if (image)
        for (int c = 0; c < C; ++c) {                                       // C <= RAS_MAX_C, checked by the host
            float a = background[c];
            if (shade)
                a = (((w[0] * attr[(size_t)corner[0] * C + c]) + (w[1] * attr[(size_t)corner[1] * C + c])) + (w[2] * attr[(size_t)corner[2] * C + c])) * z;
            image[(size_t)c * n + p] = a;
        }
}

}  // namespace
