// mesh_fusion_kernels.h -- TSDF fusion of rendered depth maps and marching tetrahedra over the fused volume (mesh_ops.hip:
// dgs_tsdf_integrate, dgs_mt_classify, dgs_mt_emit).
#pragma once
#include <hip/hip_runtime.h>

#include "mesh_common.h"

namespace {

// ---- fusion ---------------------------------------------------------------------------------------------------------------------
// A workgroup owns a brick of RX x BY x BZ voxels: 256 threads tile (y, z) -- z, the fastest axis of the volume, across the lanes,
// so the stores of a wave are four 64-byte runs -- and every thread walks RX voxels along x with their state in registers.  The
// brick projects into a patch of a few pixels squared in any one view, so the taps of a workgroup fall into a few cache lines.
constexpr int BZ = 16, BY = 16, RX = 4;

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

}  // namespace
