// libdgs_mesh_ops.so (include/dgs_mesh_ops.h): TSDF fusion of rendered depth maps, marching tetrahedra, the all-pairs
// nearest-neighbour and closest-triangle searches of the mesh metrics, the z-buffer triangle rasterizer of the mesh images and the
// connected components of the mesh clean-up, gfx950.
// Compiled with -ffp-contract=off: every fp32 operation below rounds on its own, which is what makes the result equal to the
// PyTorch statement of the same arithmetic (dgs_amd/mesh.py) instead of close to it.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/dgs_mesh_ops.h"

namespace {
thread_local std::string g_err;
int fail(int code, const std::string& m) { g_err = m; return code; }
int launched(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-2, std::string(what) + ": " + hipGetErrorString(e));
    return 0;
}

// ---- fusion ---------------------------------------------------------------------------------------------------------------------
// A workgroup owns a brick of RX x BY x BZ voxels: 256 threads tile (y, z) -- z, the fastest axis of the volume, across the lanes,
// so the stores of a wave are four 64-byte runs -- and every thread walks RX voxels along x with their state in registers.  The
// brick projects into a patch of a few pixels squared in any one view, so the taps of a workgroup fall into a few cache lines.
constexpr int BZ = 16, BY = 16, RX = 4;

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

__global__ __launch_bounds__(BZ * BY) void tsdf_integrate_kernel(
    int Nx, int Ny, int Nz, float ox, float oy, float oz, float h, int V, int H, int W, const float* __restrict__ depth,
    const float* __restrict__ rgb, const float* __restrict__ proj, float trunc, float depth_trunc, float prior_weight, int accumulate,
    float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ color) {
    const int k = blockIdx.x * BZ + threadIdx.x, j = blockIdx.y * BY + threadIdx.y, i0 = blockIdx.z * RX;
    if (k >= Nz || j >= Ny) return;
    const long long lin0 = ((long long)i0 * Ny + j) * Nz + k, sx = (long long)Ny * Nz;
    const int nr = min(RX, Nx - i0);
    float ts[RX], w[RX], cr[RX], cg[RX], cb[RX], px[RX];
#pragma unroll
    for (int r = 0; r < RX; ++r) {
        px[r] = ox + h * (float)(i0 + r);
        ts[r] = prior_weight > 0.0f ? 1.0f : 0.0f;
        w[r] = prior_weight;
        cr[r] = cg[r] = cb[r] = 0.0f;
        if (accumulate && r < nr) {
            const long long l = lin0 + r * sx;
            ts[r] = tsdf[l], w[r] = weight[l];
            cr[r] = color[3 * l], cg[r] = color[3 * l + 1], cb[r] = color[3 * l + 2];
        }
    }
    const float py = oy + h * (float)j, pz = oz + h * (float)k;
    const float Wf = (float)W, Hf = (float)H, umax = (float)(W - 2), vmax = (float)(H - 2);
    const size_t plane = (size_t)H * W;
    for (int v = 0; v < V; ++v) {
        const float* m = proj + 16 * v;   // uniform address: scalar loads
        const float bx = (py * m[4] + pz * m[8]) + m[12], by = (py * m[5] + pz * m[9]) + m[13], bw = (py * m[7] + pz * m[11]) + m[15];
        const float m0x = m[0], m0y = m[1], m0w = m[3];
        const float* dp = depth + (size_t)v * plane;
#pragma unroll
        for (int r = 0; r < RX; ++r) {
            if (r >= nr) continue;
            const float z = px[r] * m0w + bw;
            if (!(z > 0.0f)) continue;
            const float nx = (px[r] * m0x + bx) / z, ny = (px[r] * m0y + by) / z;
            if (!(nx > -1.0f && nx < 1.0f && ny > -1.0f && ny < 1.0f)) continue;
            const float u = ((nx + 1.0f) * Wf - 1.0f) / 2.0f, vv = ((ny + 1.0f) * Hf - 1.0f) / 2.0f;
            const float u0 = fminf(fmaxf(floorf(u), 0.0f), umax), v0 = fminf(fmaxf(floorf(vv), 0.0f), vmax);
            const float fu = clamp01(u - u0), fv = clamp01(vv - v0);
            const size_t a = (size_t)(int)v0 * W + (size_t)(int)u0;   // u0 in [0, W-2], v0 in [0, H-2]: a + W + 1 < H * W
            const float d00 = dp[a], d01 = dp[a + 1], d10 = dp[a + W], d11 = dp[a + W + 1];
            if (!(d00 > 0.0f && d00 <= depth_trunc && d01 > 0.0f && d01 <= depth_trunc && d10 > 0.0f && d10 <= depth_trunc && d11 > 0.0f &&
                  d11 <= depth_trunc))
                continue;
            const float gu = 1.0f - fu, gv = 1.0f - fv;
            const float d = (d00 * gu + d01 * fu) * gv + (d10 * gu + d11 * fu) * fv;
            const float sdf = d - z;
            if (!(sdf > -trunc)) continue;
            const float s = fminf(fmaxf(sdf / trunc, -1.0f), 1.0f);
            const float wn = w[r] + 1.0f;
            ts[r] = (ts[r] * w[r] + s) / wn;
            if (sdf < trunc) {
                const float* c = rgb + (size_t)v * 3 * plane + a;
                cr[r] = (cr[r] * w[r] + ((c[0] * gu + c[1] * fu) * gv + (c[W] * gu + c[W + 1] * fu) * fv)) / wn;
                c += plane;
                cg[r] = (cg[r] * w[r] + ((c[0] * gu + c[1] * fu) * gv + (c[W] * gu + c[W + 1] * fu) * fv)) / wn;
                c += plane;
                cb[r] = (cb[r] * w[r] + ((c[0] * gu + c[1] * fu) * gv + (c[W] * gu + c[W + 1] * fu) * fv)) / wn;
            }
            w[r] = wn;
        }
    }
#pragma unroll
    for (int r = 0; r < RX; ++r) {
        if (r >= nr) continue;
        const long long l = lin0 + r * sx;
        tsdf[l] = ts[r], weight[l] = w[r];
        color[3 * l] = cr[r], color[3 * l + 1] = cg[r], color[3 * l + 2] = cb[r];
    }
}

// ---- marching tetrahedra --------------------------------------------------------------------------------------------------------
// Kuhn tetrahedron t = corners {0, TC1[t], TC2[t], 7} (a chain 0 < c1 < c2 < 7 of corner sets: ascending linear index as well).
__device__ __constant__ const int TC1[6] = {1, 1, 2, 2, 4, 4};
__device__ __constant__ const int TC2[6] = {3, 5, 3, 6, 5, 6};
// Orientation of tetrahedron t = parity of its permutation: + - - + + -  (bit t set: odd)
constexpr unsigned TET_ODD = 0x26;
// Winding: for the sign pattern S (bit p set: chain position p is negative) of an EVEN tetrahedron, bit S of KEEP_EVEN says that the
// triangles as listed in the header already have their normal pointing from negative to positive; an odd tetrahedron inverts it.
constexpr unsigned KEEP_EVEN = 0x32DA;

struct Grid {
    int Nx, Ny, Nz;
    long long sx, sy;   // linear-index strides of x and y (z has stride 1)
    __device__ long long off(int c) const { return (c & 1) * sx + ((c >> 1) & 1) * sy + ((c >> 2) & 1); }
};

__device__ __forceinline__ unsigned corner_signs(const Grid& g, const float* __restrict__ tsdf, long long lin) {
    unsigned neg = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) neg |= (tsdf[lin + g.off(c)] < 0.0f ? 1u : 0u) << c;
    return neg;
}

__device__ __forceinline__ int tet_pattern(unsigned neg, int t) {
    return (neg & 1) | (((neg >> TC1[t]) & 1) << 1) | (((neg >> TC2[t]) & 1) << 2) | (((neg >> 7) & 1) << 3);
}

__global__ __launch_bounds__(256) void mt_cells_kernel(Grid g, long long n, const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                       int* __restrict__ cell_tris) {
    for (long long lin = (long long)blockIdx.x * blockDim.x + threadIdx.x; lin < n; lin += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(lin % g.Nz), j = (int)((lin / g.Nz) % g.Ny), i = (int)(lin / g.sx);
        int tris = 0;
        if (i < g.Nx - 1 && j < g.Ny - 1 && k < g.Nz - 1) {
            bool seen = true;
#pragma unroll
            for (int c = 0; c < 8; ++c) seen = seen && weight[lin + g.off(c)] > 0.0f;
            const unsigned neg = corner_signs(g, tsdf, lin);
            if (seen && neg != 0 && neg != 0xFF) {
#pragma unroll
                for (int t = 0; t < 6; ++t) {
                    const int c = __popc(tet_pattern(neg, t));
                    tris += (c == 2) ? 2 : ((c == 1 || c == 3) ? 1 : 0);
                }
            }
        }
        cell_tris[lin] = tris;
    }
}

__global__ __launch_bounds__(256) void mt_points_kernel(Grid g, long long n, const float* __restrict__ tsdf, const int* __restrict__ cell_tris,
                                                        int* __restrict__ point_verts, unsigned char* __restrict__ point_mask) {
    for (long long lin = (long long)blockIdx.x * blockDim.x + threadIdx.x; lin < n; lin += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(lin % g.Nz), j = (int)((lin / g.Nz) % g.Ny), i = (int)(lin / g.sx);
        // active flags of the up to 8 cells that have this grid point as corner o: cell = g - o
        unsigned act = 0;
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            const int ci = i - (o & 1), cj = j - ((o >> 1) & 1), ck = k - ((o >> 2) & 1);
            if (ci >= 0 && cj >= 0 && ck >= 0 && ci < g.Nx - 1 && cj < g.Ny - 1 && ck < g.Nz - 1 && cell_tris[lin - g.off(o)] > 0) act |= 1u << o;
        }
        unsigned mask = 0;
        if (act) {
            const bool neg0 = tsdf[lin] < 0.0f;
#pragma unroll
            for (int d = 1; d < 8; ++d) {
                if (i + (d & 1) >= g.Nx || j + ((d >> 1) & 1) >= g.Ny || k + ((d >> 2) & 1) >= g.Nz) continue;
                // the cells that contain the edge g -> g + d are those where g is corner o with o & d == 0
                unsigned holders = 0;
#pragma unroll
                for (int o = 0; o < 8; ++o)
                    if ((o & d) == 0) holders |= 1u << o;
                if ((act & holders) && ((tsdf[lin + g.off(d)] < 0.0f) != neg0)) mask |= 1u << (d - 1);
            }
        }
        point_mask[lin] = (unsigned char)mask;
        point_verts[lin] = __popc(mask);
    }
}

__global__ __launch_bounds__(256) void mt_vertices_kernel(Grid g, float ox, float oy, float oz, float h, const float* __restrict__ tsdf,
                                                          const float* __restrict__ color, long long n_points, const long long* __restrict__ points,
                                                          const unsigned char* __restrict__ point_mask, const long long* __restrict__ vert_incl,
                                                          float* __restrict__ vertices, float* __restrict__ vcolors) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_points) return;
    const long long lin = points[t];
    const unsigned mask = point_mask[lin];
    long long id = vert_incl[lin] - __popc(mask);
    const int k = (int)(lin % g.Nz), j = (int)((lin / g.Nz) % g.Ny), i = (int)(lin / g.sx);
    const float fa = tsdf[lin];
    const float pa[3] = {ox + h * (float)i, oy + h * (float)j, oz + h * (float)k};
    for (int d = 1; d < 8; ++d) {
        if (!((mask >> (d - 1)) & 1)) continue;
        const long long lb = lin + g.off(d);
        const float fb = tsdf[lb];
        const float s = fa / (fa - fb);
        const float pb[3] = {ox + h * (float)(i + (d & 1)), oy + h * (float)(j + ((d >> 1) & 1)), oz + h * (float)(k + ((d >> 2) & 1))};
#pragma unroll
        for (int c = 0; c < 3; ++c) vertices[3 * id + c] = pa[c] + s * (pb[c] - pa[c]);
        if (color != nullptr) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float ca = color[3 * lin + c], cb = color[3 * lb + c];
                vcolors[3 * id + c] = ca + s * (cb - ca);
            }
        }
        ++id;
    }
}

__global__ __launch_bounds__(256) void mt_faces_kernel(Grid g, const float* __restrict__ tsdf, long long n_cells, const long long* __restrict__ cells,
                                                       const int* __restrict__ cell_tris, const long long* __restrict__ tri_incl,
                                                       const unsigned char* __restrict__ point_mask, const long long* __restrict__ vert_incl,
                                                       int* __restrict__ faces) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_cells) return;
    const long long lin = cells[t];
    long long f = tri_incl[lin] - cell_tris[lin];
    const unsigned neg = corner_signs(g, tsdf, lin);
    // id of the vertex on the edge between corners a and b of this cell, a a subset of b
    auto vid = [&](int a, int b) -> int {
        const long long la = lin + g.off(a);
        const unsigned m = point_mask[la];
        const int d = a ^ b;
        return (int)(vert_incl[la] - __popc(m) + __popc(m & ((1u << (d - 1)) - 1u)));
    };
    for (int tet = 0; tet < 6; ++tet) {
        const int S = tet_pattern(neg, tet), cnt = __popc(S);
        if (cnt == 0 || cnt == 4) continue;
        const int ch[4] = {0, TC1[tet], TC2[tet], 7};
        const bool keep = (((KEEP_EVEN >> S) & 1) != 0) != (((TET_ODD >> tet) & 1) != 0);
        int q[4];
        int nt;
        if (cnt == 2) {
            int in[2], out[2], ni = 0, no = 0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if ((S >> p) & 1) in[ni++] = p; else out[no++] = p;
            }
            auto e = [&](int x, int y) { return x < y ? vid(ch[x], ch[y]) : vid(ch[y], ch[x]); };
            q[0] = e(in[0], out[0]), q[1] = e(in[0], out[1]), q[2] = e(in[1], out[1]), q[3] = e(in[1], out[0]);
            nt = 2;
        } else {
            const int lone = cnt == 1 ? S : (~S & 15);
            const int apex = __ffs(lone) - 1;
            int n = 0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (p == apex) continue;
                q[n++] = p < apex ? vid(ch[p], ch[apex]) : vid(ch[apex], ch[p]);
            }
            q[3] = q[2];
            nt = 1;
        }
        faces[3 * f] = q[0], faces[3 * f + 1] = keep ? q[1] : q[2], faces[3 * f + 2] = keep ? q[2] : q[1];
        ++f;
        if (nt == 2) {
            faces[3 * f] = q[0], faces[3 * f + 1] = keep ? q[2] : q[3], faces[3 * f + 2] = keep ? q[3] : q[2];
            ++f;
        }
    }
}

// ---- nearest neighbour ----------------------------------------------------------------------------------------------------------
// A workgroup owns NN_Q = 256 x NN_K queries (each thread NN_K of them in registers: coordinates, best d2, best index) and one slice
// of the reference set, which it walks in rounds of NN_T points.  A round is staged into LDS with coalesced loads of the raw
// [n, 3] floats and de-interleaved on the way (x | y | z planes), so the inner loop reads four points with three 16-byte LDS reads
// at an address every lane shares: a broadcast, no bank conflict, and one LDS instruction per 16 / 3 query-point pairs of a
// thread.  Scanning the slice in ascending index with a strict `<` keeps the lowest index among equal distances; across slices the
// packed (d2 bits, index) minimum does.  Per pair: 3 subtractions, 3 multiplications, 2 additions, compare, 2 selects.
constexpr int NN_THREADS = 256, NN_K = 4, NN_Q = NN_THREADS * NN_K, NN_T = 1024, NN_CHUNK = 4096;

__global__ __launch_bounds__(NN_THREADS) void nn_search_kernel(long long n_query, const float* __restrict__ query, long long n_ref,
                                                               const float* __restrict__ ref, long long ref_chunk,
                                                               unsigned long long* __restrict__ best) {
    __shared__ __attribute__((aligned(16))) float pts[3 * NN_T];
    const long long q0 = (long long)blockIdx.x * NN_Q + threadIdx.x;       // this thread's queries: q0 + k * NN_THREADS
    const long long r_begin = (long long)blockIdx.y * ref_chunk;           // the host clamps ref_chunk to n_ref: no overflow
    const long long r_end = r_begin + ref_chunk < n_ref ? r_begin + ref_chunk : n_ref;
    float qx[NN_K], qy[NN_K], qz[NN_K], bd[NN_K];
    int bi[NN_K];
#pragma unroll
    for (int k = 0; k < NN_K; ++k) {
        const long long q = q0 + (long long)k * NN_THREADS;
        const bool live = q < n_query;                                     // a thread past the end computes on zeros and stores nothing
        qx[k] = live ? query[3 * q] : 0.0f, qy[k] = live ? query[3 * q + 1] : 0.0f, qz[k] = live ? query[3 * q + 2] : 0.0f;
        bd[k] = __builtin_inff(), bi[k] = 0;
    }
    auto visit = [&](float x, float y, float z, int r) {
#pragma unroll
        for (int k = 0; k < NN_K; ++k) {
            const float dx = qx[k] - x, dy = qy[k] - y, dz = qz[k] - z;
            const float d = (dx * dx + dy * dy) + dz * dz;
            const bool less = d < bd[k];
            bd[k] = less ? d : bd[k], bi[k] = less ? r : bi[k];
        }
    };
    for (long long rs = r_begin; rs < r_end; rs += NN_T) {
        const int n = (int)(r_end - rs < NN_T ? r_end - rs : NN_T);       // points of this round: only they are staged and read
        __syncthreads();                                                   // the previous round's readers are done
        const float* src = ref + 3 * rs;
        for (int e = threadIdx.x; e < 3 * n; e += NN_THREADS) {            // 3 (rs + n) <= 3 n_ref: inside the reference array
            const int p = e / 3;
            pts[(e - 3 * p) * NN_T + p] = src[e];
        }
        __syncthreads();
        const int base = (int)(rs - r_begin);                              // index within the slice (< n_ref < 2^31)
        int j = 0;
        for (; j + 4 <= n; j += 4) {
            const float4 X = *reinterpret_cast<const float4*>(&pts[j]), Y = *reinterpret_cast<const float4*>(&pts[NN_T + j]),
                         Z = *reinterpret_cast<const float4*>(&pts[2 * NN_T + j]);
            visit(X.x, Y.x, Z.x, base + j), visit(X.y, Y.y, Z.y, base + j + 1);
            visit(X.z, Y.z, Z.z, base + j + 2), visit(X.w, Y.w, Z.w, base + j + 3);
        }
        for (; j < n; ++j) visit(pts[j], pts[NN_T + j], pts[2 * NN_T + j], base + j);
    }
#pragma unroll
    for (int k = 0; k < NN_K; ++k) {
        const long long q = q0 + (long long)k * NN_THREADS;
        if (q < n_query)
            atomicMin(&best[q], ((unsigned long long)__float_as_uint(bd[k]) << 32) | (unsigned long long)(unsigned)(r_begin + bi[k]));
    }
}

// ---- closest triangle -----------------------------------------------------------------------------------------------------------
// The shape of nn_search_kernel with a table row where that one has a point.  A workgroup owns TRI_Q = 256 x TRI_K queries (each
// thread TRI_K of them in registers: coordinates, best d2, best face) and one slice of the table, which it walks in rounds of TRI_T
// rows.  A round is a straight copy of TRI_T x 144 bytes into LDS (16-byte loads and stores, coalesced); the inner loop reads one
// row with nine 16-byte LDS reads at an address every lane shares -- a broadcast -- and evaluates it for the thread's TRI_K
// queries, 92 VALU instructions each (no fma, no division; the clamp is an output modifier of a multiply), so the LDS sees one
// instruction per 41 VALU instructions.
// Sizing: 256 rows are 36 KB, four workgroups per CU (of 160 KB) = four waves per SIMD, which is also what the registers allow
// (126 VGPRs): a broadcast row is 34 live VGPRs next to 20 of query state and the pair's temporaries.  More queries per thread
// would amortise the row further but the LDS is already idle 80 % of the time; fewer would halve the work per LDS read for nothing.
constexpr int TRI_THREADS = 256, TRI_K = 4, TRI_Q = TRI_THREADS * TRI_K, TRI_T = 256, TRI_ROW = 36, TRI_ROW4 = TRI_ROW / 4, TRI_CHUNK = 4096;

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// squared distance of P to the segment from O along e, r = 1 / dot(e, e) or 0;  (wx, wy, wz) = P - O
__device__ __forceinline__ float segment_d2(float wx, float wy, float wz, float ex, float ey, float ez, float r) {
    const float t = clamp01(dot3(wx, wy, wz, ex, ey, ez) * r);
    const float cx = wx - t * ex, cy = wy - t * ey, cz = wz - t * ez;
    return dot3(cx, cy, cz, cx, cy, cz);
}

__global__ __launch_bounds__(TRI_THREADS) void tri_search_kernel(long long n_query, const float* __restrict__ query, long long n_tri,
                                                                 const float4* __restrict__ table, long long tri_chunk,
                                                                 unsigned long long* __restrict__ best) {
    __shared__ float4 rows[TRI_T * TRI_ROW4];
    const long long q0 = (long long)blockIdx.x * TRI_Q + threadIdx.x;      // this thread's queries: q0 + k * TRI_THREADS
    const long long f_begin = (long long)blockIdx.y * tri_chunk;           // the host clamps tri_chunk to n_tri: no overflow
    const long long f_end = f_begin + tri_chunk < n_tri ? f_begin + tri_chunk : n_tri;
    float qx[TRI_K], qy[TRI_K], qz[TRI_K], bd[TRI_K];
    int bi[TRI_K];
#pragma unroll
    for (int k = 0; k < TRI_K; ++k) {
        const long long q = q0 + (long long)k * TRI_THREADS;
        const bool live = q < n_query;                                     // a thread past the end computes on zeros and stores nothing
        qx[k] = live ? query[3 * q] : 0.0f, qy[k] = live ? query[3 * q + 1] : 0.0f, qz[k] = live ? query[3 * q + 2] : 0.0f;
        bd[k] = __builtin_inff(), bi[k] = 0;
    }
    for (long long fs = f_begin; fs < f_end; fs += TRI_T) {
        const int n = (int)(f_end - fs < TRI_T ? f_end - fs : TRI_T);     // rows of this round: only they are staged and read
        __syncthreads();                                                   // the previous round's readers are done
        const float4* src = table + fs * TRI_ROW4;
        for (int e = threadIdx.x; e < n * TRI_ROW4; e += TRI_THREADS)      // (fs + n) rows <= n_tri rows: inside the table;
            rows[e] = src[e];                                              // e < TRI_T * TRI_ROW4: inside the LDS array
        __syncthreads();
        const int base = (int)(fs - f_begin);                              // index within the slice (< n_tri < 2^31)
        for (int j = 0; j < n; ++j) {
            float f[TRI_ROW];
#pragma unroll
            for (int v = 0; v < TRI_ROW4; ++v) {
                const float4 x = rows[j * TRI_ROW4 + v];
                f[4 * v] = x.x, f[4 * v + 1] = x.y, f[4 * v + 2] = x.z, f[4 * v + 3] = x.w;
            }
            // A 0..2, B 3..5, C 6..8, e0 9..11, e1 12..14, e2 15..17, n 18..20, m0 21..23, m1 24..26, m2 27..29, r0 r1 r2 rn 30..33
#pragma unroll
            for (int k = 0; k < TRI_K; ++k) {
                const float ax = qx[k] - f[0], ay = qy[k] - f[1], az = qz[k] - f[2];
                const float bx = qx[k] - f[3], by = qy[k] - f[4], bz = qz[k] - f[5];
                const float cx = qx[k] - f[6], cy = qy[k] - f[7], cz = qz[k] - f[8];
                const float s0 = segment_d2(ax, ay, az, f[9], f[10], f[11], f[30]);
                const float s1 = segment_d2(bx, by, bz, f[12], f[13], f[14], f[31]);
                const float s2 = segment_d2(cx, cy, cz, f[15], f[16], f[17], f[32]);
                const float edges = fminf(fminf(s0, s1), s2);
                const bool inside = (dot3(ax, ay, az, f[21], f[22], f[23]) >= 0.0f) & (dot3(bx, by, bz, f[24], f[25], f[26]) >= 0.0f) &
                                    (dot3(cx, cy, cz, f[27], f[28], f[29]) >= 0.0f) & (f[33] > 0.0f);
                const float h = dot3(ax, ay, az, f[18], f[19], f[20]);
                const float pl = (h * h) * f[33];
                const float d = inside ? fminf(pl, edges) : edges;
                const bool less = d < bd[k];                               // strict: the lowest face among equal distances stays
                bd[k] = less ? d : bd[k], bi[k] = less ? base + j : bi[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < TRI_K; ++k) {
        const long long q = q0 + (long long)k * TRI_THREADS;
        if (q < n_query)
            atomicMin(&best[q], ((unsigned long long)__float_as_uint(bd[k]) << 32) | (unsigned long long)(unsigned)(f_begin + bi[k]));
    }
}

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

// ---- connected components -------------------------------------------------------------------------------------------------------
// Lock-free union-find over label[] (include/dgs_mesh_ops.h states the contract).  INVARIANT: label[x] <= x at all times, and
// label[x] is a node of x's component.  init writes label[x] = x; the only write of the hook kernel is a successful
// atomicCAS(&label[hi], hi, lo) with lo < hi, which lowers the entry of a node that is a root at that instant; the compress kernel
// only replaces an entry by the node's root.  So every walk x -> label[x] -> ... strictly descends and ends after at most x steps at
// a node with label[r] == r.
// STALE READS.  The walks read with relaxed agent-scope atomic loads, which are served past the CU's L1.  Correctness does not rest
// on their freshness: whatever value a load returns was label[x] at some instant since the init launch, so it is an ancestor of x
// (or x) in x's component.  A walk over stale values therefore ends at an ancestor r of its start that looked like a root; whether
// it still is one is decided by the CAS alone, which executes at the memory side and returns the entry's true value.  If r has a
// parent by then, the CAS fails, writes nothing and returns that parent (< r), and the union goes on from there: after every failed
// CAS the larger of the two candidates is strictly smaller than before, so a thread cannot spin, however stale its loads are.
constexpr int CC_THREADS = 256, CC_GROUPS_PER_THREAD = 1, CC_MAX_BLOCKS = 1 << 22;

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int cc_find(const int* label, int x) {          // 0 <= x < n_nodes; every value read is in [0, x]
    for (int p = cc_load(label + x); p != x; p = cc_load(label + x)) x = p;
    return x;
}

__device__ __forceinline__ void cc_unite(int* label, int a, int b) {
    int ra = cc_find(label, a), rb = cc_find(label, b);
    while (ra != rb) {                                                      // equal: a and b have a common ancestor already
        const int hi = max(ra, rb), lo = min(ra, rb);
        const int old = atomicCAS(label + hi, hi, lo);
        if (old == hi) return;                                              // hi was a root and now hangs below lo
        ra = cc_find(label, old), rb = lo;                                  // old < hi is hi's true parent: go on from there
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(long long n_nodes, int* __restrict__ label) {
    for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < n_nodes; i += (long long)gridDim.x * CC_THREADS) label[i] = (int)i;
}

template <int K>
__global__ __launch_bounds__(CC_THREADS) void cc_hook_kernel(long long n_nodes, const int* __restrict__ groups, long long n_groups, int* label) {
    for (long long g = (long long)blockIdx.x * CC_THREADS + threadIdx.x; g < n_groups; g += (long long)gridDim.x * CC_THREADS) {
        int anchor = -1;                                                    // the first id of the group that lies inside [0, n_nodes)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int v = groups[g * K + j];
            if (v < 0 || v >= n_nodes) continue;                            // index guard: no address below leaves label[0, n_nodes)
            if (anchor < 0) anchor = v;
            else if (v != anchor) cc_unite(label, anchor, v);
        }
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_compress_kernel(long long n_nodes, int* label) {
    for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < n_nodes; i += (long long)gridDim.x * CC_THREADS) {
        const int p = cc_load(label + i);
        if (p == (int)i) continue;
        const int r = cc_find(label, p);
        if (r != p) __hip_atomic_store(label + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

int check_raster(const char* what, int H, int W, long long n_faces, const float* table) {
    if (H < 1 || W < 1) return fail(-1, std::string(what) + ": H and W must be >= 1");
    if ((long long)H * W > (1LL << 30)) return fail(-1, std::string(what) + ": image too large (H * W > 2^30)");
    if (n_faces < 0) return fail(-1, std::string(what) + ": negative n_faces");
    if (n_faces >= (1LL << 31)) return fail(-1, std::string(what) + ": n_faces must be below 2^31 (the face is the low 32 bits of the packed minimum)");
    if (n_faces > 0 && !table) return fail(-1, std::string(what) + ": null pointer");
    if ((size_t)table % 16 != 0) return fail(-1, std::string(what) + ": the table must be 16-byte aligned");
    return 0;
}

int check_grid(int Nx, int Ny, int Nz, const char* what) {
    if (Nx < 2 || Ny < 2 || Nz < 2) return fail(-1, std::string(what) + ": every grid dimension must be >= 2");
    return 0;
}

unsigned blocks_for(long long n, long long cap) {
    long long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}
}  // namespace

extern "C" {

int dgs_mesh_ops_abi_version(void) { return DGS_MESH_OPS_ABI_VERSION; }
const char* dgs_mesh_ops_last_error(void) { return g_err.c_str(); }

int dgs_tsdf_integrate(int Nx, int Ny, int Nz, float ox, float oy, float oz, float voxel, int V, int H, int W, const float* depth,
                       const float* rgb, const float* proj, float trunc, float depth_trunc, float prior_weight, int accumulate, float* tsdf,
                       float* weight, float* color, void* stream) {
    if (Nx < 1 || Ny < 1 || Nz < 1) return fail(-1, "dgs_tsdf_integrate: empty grid");
    if (V < 0 || H < 2 || W < 2) return fail(-1, "dgs_tsdf_integrate: views must be at least 2 x 2 pixels");
    if ((long long)H * W > (1LL << 30)) return fail(-1, "dgs_tsdf_integrate: view too large");
    if (!(trunc > 0.0f) || !(voxel > 0.0f) || !(prior_weight >= 0.0f)) return fail(-1, "dgs_tsdf_integrate: trunc and voxel must be positive, prior_weight >= 0");
    if (!tsdf || !weight || !color || (V > 0 && (!depth || !rgb || !proj))) return fail(-1, "dgs_tsdf_integrate: null pointer");
    const dim3 grid((Nz + BZ - 1) / BZ, (Ny + BY - 1) / BY, (Nx + RX - 1) / RX);
    if (grid.y > 65535u || grid.z > 65535u) return fail(-1, "dgs_tsdf_integrate: grid too large");
    hipLaunchKernelGGL(tsdf_integrate_kernel, grid, dim3(BZ, BY, 1), 0, (hipStream_t)stream, Nx, Ny, Nz, ox, oy, oz, voxel, V, H, W, depth, rgb,
                       proj, trunc, depth_trunc, prior_weight, accumulate, tsdf, weight, color);
    return launched("dgs_tsdf_integrate");
}

int dgs_mt_classify(int Nx, int Ny, int Nz, const float* tsdf, const float* weight, int* cell_tris, int* point_verts,
                    unsigned char* point_mask, void* stream) {
    if (int rc = check_grid(Nx, Ny, Nz, "dgs_mt_classify")) return rc;
    if (!tsdf || !weight || !cell_tris || !point_verts || !point_mask) return fail(-1, "dgs_mt_classify: null pointer");
    const Grid g{Nx, Ny, Nz, (long long)Ny * Nz, (long long)Nz};
    const long long n = (long long)Nx * Ny * Nz;
    const unsigned nb = blocks_for(n, 1 << 20);
    hipLaunchKernelGGL(mt_cells_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, g, n, tsdf, weight, cell_tris);
    if (int rc = launched("dgs_mt_classify (cells)")) return rc;
    hipLaunchKernelGGL(mt_points_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, g, n, tsdf, cell_tris, point_verts, point_mask);
    return launched("dgs_mt_classify (points)");
}

int dgs_mt_emit(int Nx, int Ny, int Nz, float ox, float oy, float oz, float voxel, const float* tsdf, const float* color, long long n_cells,
                const long long* cells, const int* cell_tris, const long long* tri_incl, long long n_points, const long long* points,
                const unsigned char* point_mask, const long long* vert_incl, float* vertices, float* vertex_colors, int* faces, void* stream) {
    if (int rc = check_grid(Nx, Ny, Nz, "dgs_mt_emit")) return rc;
    if (n_cells < 0 || n_points < 0) return fail(-1, "dgs_mt_emit: negative count");
    if (n_cells == 0 || n_points == 0) return 0;
    if (!tsdf || !cells || !cell_tris || !tri_incl || !points || !point_mask || !vert_incl || !vertices || !faces || (color && !vertex_colors))
        return fail(-1, "dgs_mt_emit: null pointer");
    const Grid g{Nx, Ny, Nz, (long long)Ny * Nz, (long long)Nz};
    hipLaunchKernelGGL(mt_vertices_kernel, dim3(blocks_for(n_points, 1LL << 31)), dim3(256), 0, (hipStream_t)stream, g, ox, oy, oz, voxel, tsdf, color,
                       n_points, points, point_mask, vert_incl, vertices, vertex_colors);
    if (int rc = launched("dgs_mt_emit (vertices)")) return rc;
    hipLaunchKernelGGL(mt_faces_kernel, dim3(blocks_for(n_cells, 1LL << 31)), dim3(256), 0, (hipStream_t)stream, g, tsdf, n_cells, cells, cell_tris,
                       tri_incl, point_mask, vert_incl, faces);
    return launched("dgs_mt_emit (faces)");
}

int dgs_nn_search(long long n_query, const float* query, long long n_ref, const float* ref, long long ref_chunk, unsigned long long* best,
                  void* stream) {
    if (n_query < 0) return fail(-1, "dgs_nn_search: negative n_query");
    if (n_ref < 1) return fail(-1, "dgs_nn_search: the reference set must hold at least one point (n_ref >= 1)");
    if (n_ref >= (1LL << 31)) return fail(-1, "dgs_nn_search: n_ref must be below 2^31 (the index is the low 32 bits of the packed minimum)");
    if (ref_chunk < 1) return fail(-1, "dgs_nn_search: ref_chunk must be >= 1");
    if (!ref || (n_query > 0 && (!query || !best))) return fail(-1, "dgs_nn_search: null pointer");
    if (n_query == 0) return 0;
    if (ref_chunk > n_ref) ref_chunk = n_ref;
    const long long slices = (n_ref + ref_chunk - 1) / ref_chunk, blocks = (n_query + NN_Q - 1) / NN_Q;
    if (slices > 65535) return fail(-1, "dgs_nn_search: more than 65535 slices: raise ref_chunk");
    if (blocks > 0x7FFFFFFFLL) return fail(-1, "dgs_nn_search: too many queries for one launch");
    hipError_t e = hipMemsetAsync(best, 0xFF, (size_t)n_query * sizeof(unsigned long long), (hipStream_t)stream);
    if (e != hipSuccess) return fail(-2, std::string("dgs_nn_search (init): ") + hipGetErrorString(e));
    hipLaunchKernelGGL(nn_search_kernel, dim3((unsigned)blocks, (unsigned)slices), dim3(NN_THREADS), 0, (hipStream_t)stream, n_query, query, n_ref,
                       ref, ref_chunk, best);
    return launched("dgs_nn_search");
}

int dgs_nn_layout(int out[3]) {
    if (!out) return fail(-1, "dgs_nn_layout: null pointer");
    out[0] = NN_Q, out[1] = NN_T, out[2] = NN_CHUNK;
    return 0;
}

int dgs_tri_search(long long n_query, const float* query, long long n_tri, const float* table, long long tri_chunk, unsigned long long* best,
                   void* stream) {
    if (n_query < 0) return fail(-1, "dgs_tri_search: negative n_query");
    if (n_tri < 1) return fail(-1, "dgs_tri_search: the table must hold at least one triangle (n_tri >= 1)");
    if (n_tri >= (1LL << 31)) return fail(-1, "dgs_tri_search: n_tri must be below 2^31 (the face is the low 32 bits of the packed minimum)");
    if (tri_chunk < 1) return fail(-1, "dgs_tri_search: tri_chunk must be >= 1");
    if (!table || (n_query > 0 && (!query || !best))) return fail(-1, "dgs_tri_search: null pointer");
    if ((size_t)table % 16 != 0) return fail(-1, "dgs_tri_search: the table must be 16-byte aligned");
    if (n_query == 0) return 0;
    if (tri_chunk > n_tri) tri_chunk = n_tri;
    const long long slices = (n_tri + tri_chunk - 1) / tri_chunk, blocks = (n_query + TRI_Q - 1) / TRI_Q;
    if (slices > 65535) return fail(-1, "dgs_tri_search: more than 65535 slices: raise tri_chunk");
    if (blocks > 0x7FFFFFFFLL) return fail(-1, "dgs_tri_search: too many queries for one launch");
    hipError_t e = hipMemsetAsync(best, 0xFF, (size_t)n_query * sizeof(unsigned long long), (hipStream_t)stream);
    if (e != hipSuccess) return fail(-2, std::string("dgs_tri_search (init): ") + hipGetErrorString(e));
    hipLaunchKernelGGL(tri_search_kernel, dim3((unsigned)blocks, (unsigned)slices), dim3(TRI_THREADS), 0, (hipStream_t)stream, n_query, query, n_tri,
                       reinterpret_cast<const float4*>(table), tri_chunk, best);
    return launched("dgs_tri_search");
}

int dgs_tri_layout(int out[4]) {
    if (!out) return fail(-1, "dgs_tri_layout: null pointer");
    out[0] = TRI_Q, out[1] = TRI_T, out[2] = TRI_CHUNK, out[3] = TRI_ROW;
    return 0;
}

int dgs_mesh_raster(long long n_faces, const float* table, const int* list, long long n_list, int path, int H, int W,
                    unsigned long long* best, int clear, void* stream) {
    if (int rc = check_raster("dgs_mesh_raster", H, W, n_faces, table)) return rc;
    if (n_list < 0) return fail(-1, "dgs_mesh_raster: negative n_list");
    if (n_list >= (1LL << 31)) return fail(-1, "dgs_mesh_raster: n_list must be below 2^31");
    if (path != 0 && path != 1) return fail(-1, "dgs_mesh_raster: path must be 0 (small boxes) or 1 (large boxes)");
    if (!best || (n_list > 0 && (!list || !table))) return fail(-1, "dgs_mesh_raster: null pointer");
    if (clear) {
        hipError_t e = hipMemsetAsync(best, 0xFF, (size_t)H * W * sizeof(unsigned long long), (hipStream_t)stream);
        if (e != hipSuccess) return fail(-2, std::string("dgs_mesh_raster (clear): ") + hipGetErrorString(e));
    }
    if (n_list == 0 || n_faces == 0) return 0;
    const float4* rows = reinterpret_cast<const float4*>(table);
    if (path == 0) {
        hipLaunchKernelGGL(raster_small_kernel, dim3((unsigned)((n_list + RAS_THREADS - 1) / RAS_THREADS)), dim3(RAS_THREADS), 0, (hipStream_t)stream,
                           n_faces, rows, list, n_list, H, W, best);
        return launched("dgs_mesh_raster (small)");
    }
    // few large faces: several workgroups per face, each a stripe of its rows; many: one each.  The result does not depend on it.
    long long stripes = RAS_TARGET_GROUPS / n_list, rows_of_tiles = ((long long)H + RAS_TILE_Y - 1) / RAS_TILE_Y;
    stripes = stripes < 1 ? 1 : (stripes > RAS_MAX_STRIPES ? RAS_MAX_STRIPES : stripes);
    if (stripes > rows_of_tiles) stripes = rows_of_tiles;
    // (a launch of 2^32 threads or more along x is refused: above RAS_MAX_GROUPS faces a workgroup takes several of them in turn)
    const long long groups = n_list < RAS_MAX_GROUPS ? n_list : RAS_MAX_GROUPS;
    hipLaunchKernelGGL(raster_large_kernel, dim3((unsigned)groups, (unsigned)stripes), dim3(RAS_THREADS), 0, (hipStream_t)stream, n_faces, rows, list,
                       n_list, H, W, best);
    return launched("dgs_mesh_raster (large)");
}

int dgs_mesh_resolve(int H, int W, const unsigned long long* best, long long n_faces, const float* table, const int* faces,
                     long long n_vertices, const float* attr, int C, const float* background, int* face_id, float* depth, float* bary,
                     float* image, void* stream) {
    if (int rc = check_raster("dgs_mesh_resolve", H, W, n_faces, table)) return rc;
    if (n_vertices < 0 || n_vertices >= (1LL << 31)) return fail(-1, "dgs_mesh_resolve: n_vertices must be in [0, 2^31)");
    if (C < 0 || C > RAS_MAX_C) return fail(-1, "dgs_mesh_resolve: C must be in [0, " + std::to_string(RAS_MAX_C) + "]");
    if (!best) return fail(-1, "dgs_mesh_resolve: null pointer");
    if (C > 0 && (!background || !image || (n_faces > 0 && !faces) || (n_vertices > 0 && !attr))) return fail(-1, "dgs_mesh_resolve: null pointer");
    const size_t n = (size_t)H * W;
    hipLaunchKernelGGL(raster_resolve_kernel, dim3((unsigned)((n + RAS_THREADS - 1) / RAS_THREADS)), dim3(RAS_THREADS), 0, (hipStream_t)stream, H, W, best,
                       n_faces, reinterpret_cast<const float4*>(table), faces, n_vertices, attr, C, background, face_id, depth, bary,
                       C > 0 ? image : nullptr);
    return launched("dgs_mesh_resolve");
}

int dgs_mesh_raster_layout(int out[4]) {
    if (!out) return fail(-1, "dgs_mesh_raster_layout: null pointer");
    out[0] = RAS_SMALL_AREA, out[1] = RAS_THREADS, out[2] = RAS_ROW, out[3] = RAS_MAX_C;
    return 0;
}

int dgs_cc_labels(long long n_nodes, const int* groups, long long n_groups, int k, int* label, void* stream) {
    if (k != 2 && k != 3) return fail(-1, "dgs_cc_labels: k must be 2 or 3");
    if (n_nodes < 0 || n_groups < 0) return fail(-1, "dgs_cc_labels: negative count");
    if (n_nodes >= (1LL << 31)) return fail(-1, "dgs_cc_labels: n_nodes must be below 2^31 (labels are int32)");
    if ((n_nodes > 0 && !label) || (n_groups > 0 && !groups)) return fail(-1, "dgs_cc_labels: null pointer");
    if (n_nodes == 0) return 0;
    const long long per_block = (long long)CC_THREADS * CC_GROUPS_PER_THREAD;
    auto blocks = [&](long long n) { const long long b = (n + per_block - 1) / per_block; return dim3((unsigned)(b > CC_MAX_BLOCKS ? CC_MAX_BLOCKS : b)); };
    hipLaunchKernelGGL(cc_init_kernel, blocks(n_nodes), dim3(CC_THREADS), 0, (hipStream_t)stream, n_nodes, label);
    if (int rc = launched("dgs_cc_labels (init)")) return rc;
    if (n_groups == 0) return 0;
    if (k == 2)
        hipLaunchKernelGGL(cc_hook_kernel<2>, blocks(n_groups), dim3(CC_THREADS), 0, (hipStream_t)stream, n_nodes, groups, n_groups, label);
    else
        hipLaunchKernelGGL(cc_hook_kernel<3>, blocks(n_groups), dim3(CC_THREADS), 0, (hipStream_t)stream, n_nodes, groups, n_groups, label);
    if (int rc = launched("dgs_cc_labels (hook)")) return rc;
    hipLaunchKernelGGL(cc_compress_kernel, blocks(n_nodes), dim3(CC_THREADS), 0, (hipStream_t)stream, n_nodes, label);
    return launched("dgs_cc_labels (compress)");
}

int dgs_cc_layout(int out[2]) {
    if (!out) return fail(-1, "dgs_cc_layout: null pointer");
    out[0] = CC_THREADS, out[1] = CC_GROUPS_PER_THREAD;
    return 0;
}

}  // extern "C"
