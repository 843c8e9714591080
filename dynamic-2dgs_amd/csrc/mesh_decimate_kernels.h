// mesh_decimate_kernels.h -- the quadric edge collapse in rounds of the mesh decimation (mesh_ops.hip: dgs_decimate_quadrics, _edges,
// _select, _apply).
// include/dgs_mesh_ops.h states every step; dgs_amd/mesh_decimate.py states the same arithmetic in PyTorch.  The quadric rows are
// int64 sums (exact in any order), everything fp64 below is written operation by operation (-ffp-contract=off), and the selection
// is decided by 64-bit atomic minima of distinct keys, whose result does not depend on the order in which they land.
// SHAPE.  A thread per face (quadrics, re-indexing), per edge (cost / placement / validity, the selection passes) or per selected
// edge (apply).  The edge kernel is the heavy one: two 10-column int64 rows, an fp64 3x3 solve, a merge of two adjacency rows and a
// walk over the faces of both endpoints (about 12 faces, 9 floats each).  All of its reads are gathers at addresses the mesh
// decides; marching tetrahedra numbers vertices by grid key, so the rows of an edge's endpoints and of their faces lie in nearby
// lines and the L2 serves most of them.  A hub of thousands of faces is one thread's loop: correct, and as slow as that sounds.
// GUARDS.  Every id read from a buffer is range-checked before an address is formed from it, and every row range is clamped to its
// array: an edge, a face or a selected entry with an id outside its range computes nothing and writes its neutral output.
#pragma once
#include "mesh_common.h"

namespace {

constexpr int DEC_THREADS = 256, DEC_ITEMS_PER_THREAD = 1, DEC_ROW = 10, DEC_Q_MAX = 40, DEC_Q_BUDGET = 59, DEC_W_MAX = 16;
constexpr int DEC_LAMBDA_EXP = QUADRIC_LAMBDA_EXP, DEC_MIN_VALENCE = 5, DEC_LEN_BITS = 28, DEC_FLAG_LOCKED = 1, DEC_FLAG_BOUNDARY = 2;
constexpr unsigned long long DEC_NO_KEY = 0x7FFFFFFFFFFFFFFFull;

__device__ __forceinline__ unsigned long long dec_key(float cost, long long edge) {
    unsigned h = (unsigned)edge * 0x9E3779B1u;              // a bijection of the 32-bit integers: equal costs are ordered pseudo-randomly
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    return ((unsigned long long)__float_as_uint(cost) << 32) | h;
}

__global__ __launch_bounds__(DEC_THREADS) void dec_quadric_kernel(long long n_faces, const int* __restrict__ faces, long long n_vertices,
                                                                  const float* __restrict__ pos, float mean_len, double scale,
                                                                  long long* __restrict__ rows) {
    const long long i = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (i >= n_faces) return;
    const int f[3] = {faces[3 * i], faces[3 * i + 1], faces[3 * i + 2]};
    if (!in_range(f[0], n_vertices) || !in_range(f[1], n_vertices) || !in_range(f[2], n_vertices)) return;   // index guard
    float p[3][3], nf[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int a = 0; a < 3; ++a) p[c][a] = pos[3 * (long long)f[c] + a];
    const float l = face_normal(p, nf);
    if (!(l > 0.0f && l < INFINITY)) return;                                   // a face without area counts for nothing
    const double n[3] = {(double)(nf[0] / l), (double)(nf[1] / l), (double)(nf[2] / l)};
    const double w = (double)fminf(l / mean_len, (float)DEC_W_MAX);
    const double d = -((n[0] * (double)p[0][0] + n[1] * (double)p[0][1]) + n[2] * (double)p[0][2]), wd = w * d;
    long long v[DEC_ROW];
    quadric_fixed(w, wd, n, scale, v);
    v[9] = fixed_round((wd * d) * scale);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < DEC_ROW; ++k)
            if (v[k] != 0) atomicAdd((unsigned long long*)(rows + (long long)f[c] * DEC_ROW + k), (unsigned long long)v[k]);
}

__global__ __launch_bounds__(DEC_THREADS) void dec_edge_kernel(long long n_vertices, const float* __restrict__ pos, const long long* __restrict__ rows,
                                                               const unsigned char* __restrict__ flags, long long n_faces,
                                                               const int* __restrict__ faces, long long n_edges, const int* __restrict__ edges,
                                                               const long long* __restrict__ adj_offsets, const int* __restrict__ adj, long long n_adj,
                                                               const long long* __restrict__ vf_offsets, const int* __restrict__ vf, long long n_vf,
                                                               double inv_scale, float max_cost, float* __restrict__ cost,
                                                               float* __restrict__ place, unsigned char* __restrict__ valid) {
    const long long e = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (e >= n_edges) return;
    const int u = edges[e], v = edges[n_edges + e], cnt = edges[2 * n_edges + e], o0 = edges[3 * n_edges + e], o1 = edges[4 * n_edges + e];
    float c_out = 0.0f, x_out[3] = {0.0f, 0.0f, 0.0f};
    bool ok = false;
    const bool ids = in_range(u, n_vertices) && in_range(v, n_vertices) && u != v;                             // index guard
    const bool lu = ids && (flags[u] & DEC_FLAG_LOCKED), lv = ids && (flags[v] & DEC_FLAG_LOCKED);
    if (ids && !(lu && lv)) {
        // (b) cost and placement
        double pu[3], pv[3], mid[3], r[DEC_ROW], x[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) pu[a] = (double)pos[3 * (long long)u + a], pv[a] = (double)pos[3 * (long long)v + a], mid[a] = (pu[a] + pv[a]) * 0.5;
#pragma unroll
        for (int k = 0; k < DEC_ROW; ++k) r[k] = (double)(rows[(long long)u * DEC_ROW + k] + rows[(long long)v * DEC_ROW + k]);
        const double a00 = r[0], a01 = r[1], a02 = r[2], a11 = r[3], a12 = r[4], a22 = r[5];
        const double A[6] = {a00, a01, a02, a11, a12, a22}, rhs[3] = {r[6], r[7], r[8]};
        double t, det, y[3];
        quadric_solve(A, rhs, mid, t, det, y);
        const double rad = (fabs(pv[0] - pu[0]) + fabs(pv[1] - pu[1])) + fabs(pv[2] - pu[2]);
        const bool good = t > 0.0 && det > 0.0 && det < (double)INFINITY && fabs(y[0] - mid[0]) <= rad && fabs(y[1] - mid[1]) <= rad &&
                          fabs(y[2] - mid[2]) <= rad;                                                       // a NaN fails
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            x_out[a] = (float)(lu ? pu[a] : (lv ? pv[a] : (good ? y[a] : mid[a])));
            x[a] = (double)x_out[a];                                                                        // the cost of where the vertex will really be
        }
        const double q0 = (a00 * x[0] + a01 * x[1]) + a02 * x[2], q1 = (a01 * x[0] + a11 * x[1]) + a12 * x[2], q2 = (a02 * x[0] + a12 * x[1]) + a22 * x[2];
        const double raw = (((x[0] * q0 + x[1] * q1) + x[2] * q2) + 2.0 * ((r[6] * x[0] + r[7] * x[1]) + r[8] * x[2])) + r[9];
        c_out = (float)((raw > 0.0 ? raw : 0.0) * inv_scale);
        ok = raw == raw && c_out <= max_cost;
        // (c) validity
        if (ok) {
            const bool rim_u = flags[u] & DEC_FLAG_BOUNDARY, rim_v = flags[v] & DEC_FLAG_BOUNDARY;
            ok = cnt <= 2 && o0 != o1 && !(cnt == 2 && rim_u && rim_v);
            const int opp[2] = {o0, o1};
#pragma unroll
            for (int k = 0; k < 2; ++k) {                                                                   // valence
                if (opp[k] < 0) continue;
                if (!in_range(opp[k], n_vertices)) { ok = false; continue; }
                long long b, en;
                csr_row(adj_offsets, opp[k], n_adj, b, en);
                ok = ok && en - b >= ((flags[opp[k]] & DEC_FLAG_BOUNDARY) ? 3 : DEC_MIN_VALENCE);
            }
        }
        if (ok) {                                                                                           // link: a merge of two ascending rows
            long long a, ae, b, be;
            csr_row(adj_offsets, u, n_adj, a, ae);
            csr_row(adj_offsets, v, n_adj, b, be);
            int n_common = 0, n_bad = 0;
            while (a < ae && b < be) {                                                                      // at most (ae - a) + (be - b) <= 2 n_adj steps
                const int s = adj[a], w = adj[b];
                if (s == w) {
                    ++n_common;
                    n_bad += s != o0 && s != o1;
                    ++a, ++b;
                } else if (s < w) ++a;
                else ++b;
            }
            ok = n_common == cnt && n_bad == 0;
        }
        for (int side = 0; side < 2 && ok; ++side) {                                                        // flip: the faces at u, then at v
            long long b, en;
            csr_row(vf_offsets, side ? v : u, n_vf, b, en);
            for (long long k = b; k < en && ok; ++k) {
                const int g = vf[k];
                if (!in_range(g, n_faces)) { ok = false; break; }
                const int f[3] = {faces[3 * (long long)g], faces[3 * (long long)g + 1], faces[3 * (long long)g + 2]};
                if (!in_range(f[0], n_vertices) || !in_range(f[1], n_vertices) || !in_range(f[2], n_vertices)) { ok = false; break; }
                const bool has_u = f[0] == u || f[1] == u || f[2] == u, has_v = f[0] == v || f[1] == v || f[2] == v;
                if (has_u && has_v) continue;                                                               // the face goes with the edge
                double p[3][3], q[3][3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const bool moves = f[c] == u || f[c] == v;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        p[c][a] = (double)pos[3 * (long long)f[c] + a];
                        q[c][a] = moves ? x[a] : p[c][a];
                    }
                }
                const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]}, e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
                const double g1[3] = {q[1][0] - q[0][0], q[1][1] - q[0][1], q[1][2] - q[0][2]}, g2[3] = {q[2][0] - q[0][0], q[2][1] - q[0][1], q[2][2] - q[0][2]};
                double n0[3], n1[3];
                cross3(e1, e2, n0);
                cross3(g1, g2, n1);
                ok = (n0[0] * n1[0] + n0[1] * n1[1]) + n0[2] * n1[2] > 0.0;                                 // zero area afterwards, or a NaN, fails
            }
        }
    }
    cost[e] = c_out;
#pragma unroll
    for (int a = 0; a < 3; ++a) place[3 * e + a] = x_out[a];
    valid[e] = ok ? 1 : 0;
}

__global__ __launch_bounds__(DEC_THREADS) void dec_fill_kernel(long long n, unsigned long long* __restrict__ m, unsigned long long value) {
    const long long i = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (i < n) m[i] = value;
}

// The 64-bit atomic minimum behind a plain load: entries only fall during a launch, so a stale read is too large and costs an atomic
// that changes nothing -- never a missed one.
__device__ __forceinline__ void dec_min(unsigned long long* p, unsigned long long key) {
    if (key < *p) atomicMin(p, key);
}

// pass 1 (PASS == 1): m1[x] = min of the keys of the competing edges at x.  pass 2 (PASS == 2), over ALL edges, m2 a copy of m1:
// m2[x] = min(m1[x], m1[y] for y adjacent to x).  pass 3: selected iff competing and m2[u] == m2[v] == key.
template <int PASS>
__global__ __launch_bounds__(DEC_THREADS) void dec_select_kernel(long long n_vertices, long long n_edges, const int* __restrict__ edges,
                                                                 const float* __restrict__ cost, const unsigned char* __restrict__ compete,
                                                                 unsigned long long* m1, unsigned long long* m2, unsigned char* __restrict__ selected) {
    const long long e = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (e >= n_edges) return;
    const int u = edges[e], v = edges[n_edges + e];
    const bool ids = in_range(u, n_vertices) && in_range(v, n_vertices);                                        // index guard
    if (PASS == 1) {
        if (!ids || !compete[e]) return;
        const unsigned long long key = dec_key(cost[e], e);
        dec_min(m1 + u, key);
        dec_min(m1 + v, key);
    } else if (PASS == 2) {
        if (!ids) return;
        dec_min(m2 + u, m1[v]);
        dec_min(m2 + v, m1[u]);
    } else {
        bool s = false;
        if (ids && compete[e]) {
            const unsigned long long key = dec_key(cost[e], e);
            s = m2[u] == key && m2[v] == key;
        }
        selected[e] = s ? 1 : 0;
    }
}

__global__ __launch_bounds__(DEC_THREADS) void dec_iota_kernel(long long n, int* __restrict__ vmap) {
    const long long i = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (i < n) vmap[i] = (int)i;
}

// A thread per selected edge.  The selected edges share no endpoint, so no two threads touch one vertex; a thread reads everything
// it needs of both endpoints before it writes.  (A list that names an edge twice would write the same values twice.)
__global__ __launch_bounds__(DEC_THREADS) void dec_collapse_kernel(long long n_vertices, float* pos, long long* rows, float* colors,
                                                                   const unsigned char* __restrict__ flags, unsigned char* moved, int* vmap,
                                                                   long long n_edges, const int* __restrict__ edges, const float* __restrict__ place,
                                                                   long long n_sel, const int* __restrict__ sel) {
    const long long i = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (i >= n_sel) return;
    const int e = sel[i];
    if (!in_range(e, n_edges)) return;                                                                        // index guard
    const int u = edges[e], v = edges[n_edges + e];
    if (!in_range(u, n_vertices) || !in_range(v, n_vertices) || u == v) return;
    const bool lu = flags[u] & DEC_FLAG_LOCKED, lv = flags[v] & DEC_FLAG_LOCKED;
    const int s = lv && !lu ? v : u, d = lv && !lu ? u : v;             // the survivor: the smaller id, unless only the larger one is locked
    float x[3], pu[3], pv[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = place[3 * (long long)e + a], pu[a] = pos[3 * (long long)u + a], pv[a] = pos[3 * (long long)v + a];
    long long sum[DEC_ROW];
#pragma unroll
    for (int k = 0; k < DEC_ROW; ++k) sum[k] = rows[(long long)u * DEC_ROW + k] + rows[(long long)v * DEC_ROW + k];
    if (colors) {
        const double dl[3] = {(double)pv[0] - (double)pu[0], (double)pv[1] - (double)pu[1], (double)pv[2] - (double)pu[2]};
        const double xr[3] = {(double)x[0] - (double)pu[0], (double)x[1] - (double)pu[1], (double)x[2] - (double)pu[2]};
        const double tt = ((xr[0] * dl[0] + xr[1] * dl[1]) + xr[2] * dl[2]) / ((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]);
        const float t = (float)(tt > 0.0 ? (tt < 1.0 ? tt : 1.0) : 0.0);                                    // a NaN counts as 0
        float c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float cu = colors[3 * (long long)u + a], cv = colors[3 * (long long)v + a];
            c[a] = cu + t * (cv - cu);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) colors[3 * (long long)s + a] = c[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) pos[3 * (long long)s + a] = x[a];
#pragma unroll
    for (int k = 0; k < DEC_ROW; ++k) rows[(long long)s * DEC_ROW + k] = sum[k];
    if (!(lu || lv)) moved[s] = 1;
    vmap[d] = s;
}

__global__ __launch_bounds__(DEC_THREADS) void dec_reindex_kernel(long long n_faces, int* __restrict__ faces, long long n_vertices,
                                                                  const int* __restrict__ vmap, unsigned char* __restrict__ keep) {
    const long long i = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (i >= n_faces) return;
    int g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int id = faces[3 * i + c];
        g[c] = in_range(id, n_vertices) ? vmap[id] : id;                                                      // index guard: such an id stays as it is
        faces[3 * i + c] = g[c];
    }
    keep[i] = g[0] != g[1] && g[1] != g[2] && g[2] != g[0];
}

}  // namespace
