// mesh_fill_kernels.h -- the list ranking, loop sums and ring emission of the mesh hole filling (mesh_ops.hip: dgs_fill_rank,
// dgs_fill_rim, dgs_fill_emit).
// include/dgs_mesh_ops.h states every step; dgs_amd/mesh_fill.py states the same arithmetic in PyTorch.  The ranks are integers, the
// sums of a loop are int64 fixed-point sums (exact in any order, combined on chip by sum_combine: neighbouring rim slots share a
// loop), and everything fp64 below is written operation by operation (-ffp-contract=off).
// SHAPE.  A thread per boundary half-edge (ranks), per rim slot (sums, smoothed rim), per new vertex or per new face (emission), over
// arrays in rank order: a loop's slots, vertices and faces are contiguous, so a wave reads a few rows of the loop and ring tables
// and neighbouring rows of S.  No kernel waits for another workgroup and no loop walks a list: the only loop is the 9 taps.
// GUARDS.  Every id and offset read from a buffer is range-checked before an address is formed from it; an item that fails a check
// writes its neutral output (rank -1, zeros, the face (0, 0, 0)).  A malformed successor table gives wrong ranks, never a hang:
// the number of rounds is an argument.
#pragma once
#include "mesh_common.h"

namespace {

constexpr int FILL_THREADS = 256, FILL_ITEMS_PER_THREAD = 1, FILL_POS_BITS = 30, FILL_NRM_BITS = 28, FILL_COL_BITS = 24;
constexpr int FILL_RING_COLS = 10, FILL_TAPS = 9, FILL_MAX_ROUNDS = 31, FILL_SUM_COLS = 9;
static_assert(FILL_THREADS == SUM_THREADS, "sum_combine is built for the workgroup fill_rim_kernel launches with");
// columns of a row of the ring table
constexpr int FR_LOOP = 0, FR_K = 1, FR_R = 2, FR_N = 3, FR_CNT = 4, FR_VBASE = 5, FR_PCNT = 6, FR_PBASE = 7, FR_FBASE = 8, FR_NF = 9;

// The packed entry of the pointer jumping: next node << 32 | distance to it.
__global__ __launch_bounds__(FILL_THREADS) void fill_rank_init_kernel(long long n_nodes, const int* __restrict__ succ,
                                                                      const int* __restrict__ leader, unsigned long long* __restrict__ out) {
    const long long h = (long long)blockIdx.x * FILL_THREADS + threadIdx.x;
    if (h >= n_nodes) return;
    const int s = succ[h], l = leader[h];
    // not ranked, a successor outside the table, or the node in front of the leader (the cut): the end of a list
    const bool end = l < 0 || !in_range(s, n_nodes) || s == l;
    out[h] = end ? (unsigned long long)h << 32 : ((unsigned long long)(unsigned)s << 32) | 1ull;
}

__global__ __launch_bounds__(FILL_THREADS) void fill_rank_round_kernel(long long n_nodes, const unsigned long long* __restrict__ in,
                                                                       unsigned long long* __restrict__ out) {
    const long long h = (long long)blockIdx.x * FILL_THREADS + threadIdx.x;
    if (h >= n_nodes) return;
    const unsigned long long e = in[h];
    const unsigned long long nx = e >> 32;
    if (nx >= (unsigned long long)n_nodes) { out[h] = e; return; }                                          // index guard (init writes no such entry)
    const unsigned long long f = in[nx];
    out[h] = (f & 0xFFFFFFFF00000000ull) | ((e + f) & 0xFFFFFFFFull);
}

__global__ __launch_bounds__(FILL_THREADS) void fill_rank_final_kernel(long long n_nodes, const int* __restrict__ leader,
                                                                       const unsigned long long* __restrict__ in, int* __restrict__ rank) {
    const long long h = (long long)blockIdx.x * FILL_THREADS + threadIdx.x;
    if (h >= n_nodes) return;
    const int l = leader[h];
    rank[h] = l < 0 ? -1 : ((long long)l == h ? 0 : (int)((in[h] + 1ull) & 0x7FFFFFFFull));
}

struct FillFrame { double centre[3], scale, inv_scale; };

__device__ __forceinline__ double fill_clamp01(float c) { return (double)(c > 0.0f ? (c < 1.0f ? c : 1.0f) : 0.0f); }       // NaN counts as 0

// the rim range [off, off + n) of loop l, or false
__device__ __forceinline__ bool fill_loop(const long long* __restrict__ offsets, int l, long long n_loops, long long n_rim, long long& off, long long& n) {
    if (!in_range(l, n_loops)) return false;
    off = offsets[l], n = offsets[l + 1] - off;
    return off >= 0 && n >= 3 && n <= n_rim && off <= n_rim - n;
}

__global__ __launch_bounds__(FILL_THREADS) void fill_rim_kernel(long long n_vertices, const float* __restrict__ vertices, const float* __restrict__ colors,
                                                                long long n_rim, const int* __restrict__ loop_vertices, const int* __restrict__ rim_loop,
                                                                long long n_loops, const long long* __restrict__ loop_offsets, FillFrame fr,
                                                                double* __restrict__ S, double* __restrict__ SC, long long* __restrict__ rows) {
    __shared__ SumShared<FILL_SUM_COLS> sh;
    const long long b = (long long)blockIdx.x * FILL_THREADS + threadIdx.x;
    int key = -1;
    long long v[FILL_SUM_COLS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double s[3] = {0.0, 0.0, 0.0}, sc[3] = {0.0, 0.0, 0.0};
    if (b < n_rim) {
        const int l = rim_loop[b];
        long long off, n;
        bool ok = fill_loop(loop_offsets, l, n_loops, n_rim, off, n) && b >= off && b - off < n;
        if (ok) {
            const long long i = b - off;
            const double w[FILL_TAPS] = {1.0 / 256, 8.0 / 256, 28.0 / 256, 56.0 / 256, 70.0 / 256, 56.0 / 256, 28.0 / 256, 8.0 / 256, 1.0 / 256};
            double p0[3] = {0.0, 0.0, 0.0}, p1[3] = {0.0, 0.0, 0.0}, c0[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int t = 0; t < FILL_TAPS; ++t) {
                const long long at = ((i + (t - 4)) % n + n) % n;
                const int r = loop_vertices[off + at];
                if (!in_range(r, n_vertices)) { ok = false; continue; }                                       // index guard
                double p[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    p[a] = ((double)vertices[3 * (long long)r + a] - fr.centre[a]) * fr.scale;
                    s[a] = t == 0 ? w[0] * p[a] : s[a] + w[t] * p[a];
                    if (t == 4) p0[a] = p[a];
                    if (t == 5) p1[a] = p[a];
                }
                if (colors) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const double c = fill_clamp01(colors[3 * (long long)r + a]);
                        sc[a] = t == 0 ? w[0] * c : sc[a] + w[t] * c;
                        if (t == 4) c0[a] = c;
                    }
                }
            }
            if (ok) {
                key = l;
                const double pos = (double)(1 << FILL_POS_BITS), nrm = (double)(1 << FILL_NRM_BITS), col = (double)(1 << FILL_COL_BITS);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int y = (a + 1) % 3, z = (a + 2) % 3;
                    v[a] = (long long)rint(p0[a] * pos);
                    v[3 + a] = (long long)rint(((p0[y] - p1[y]) * (p0[z] + p1[z])) * nrm);                    // Newell
                    v[6 + a] = (long long)rint(c0[a] * col);
                }
            } else {
                s[0] = s[1] = s[2] = sc[0] = sc[1] = sc[2] = 0.0;
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            S[3 * b + a] = s[a];
            if (SC) SC[3 * b + a] = sc[a];
        }
    }
    sum_combine<FILL_SUM_COLS, 0>(sh, key, v, n_loops, rows);
}

// What the two emission kernels share: the row of the ring table an item belongs to and the rim range of its loop.
struct FillRing { int l, k, R, cnt, vbase, pcnt, pbase, fbase, nf; long long off, n; };

__device__ __forceinline__ bool fill_ring(const int* __restrict__ rings, long long n_rings, int rid, const long long* __restrict__ loop_offsets,
                                          long long n_loops, long long n_rim, FillRing& g) {
    if (!in_range(rid, n_rings)) return false;
    const int* row = rings + (long long)rid * FILL_RING_COLS;
    g.l = row[FR_LOOP], g.k = row[FR_K], g.R = row[FR_R], g.cnt = row[FR_CNT], g.vbase = row[FR_VBASE], g.pcnt = row[FR_PCNT];
    g.pbase = row[FR_PBASE], g.fbase = row[FR_FBASE], g.nf = row[FR_NF];
    return fill_loop(loop_offsets, g.l, n_loops, n_rim, g.off, g.n) && g.n == (long long)row[FR_N] && g.k >= 1 && g.k <= g.R;
}

__global__ __launch_bounds__(FILL_THREADS) void fill_vertex_kernel(long long n_old, long long n_new, const int* __restrict__ vert_ring,
                                                                   long long n_rings, const int* __restrict__ rings, long long n_loops,
                                                                   const long long* __restrict__ loop_offsets, long long n_rim,
                                                                   const long long* __restrict__ rows, const double* __restrict__ S,
                                                                   const double* __restrict__ SC, FillFrame fr, float* __restrict__ vertices_out,
                                                                   float* __restrict__ colors_out) {
    const long long q = (long long)blockIdx.x * FILL_THREADS + threadIdx.x;
    if (q >= n_new) return;
    float x[3] = {0.0f, 0.0f, 0.0f}, c[3] = {0.0f, 0.0f, 0.0f};
    FillRing g = {};
    const bool ok = fill_ring(rings, n_rings, vert_ring[q], loop_offsets, n_loops, n_rim, g);
    const long long j = n_old + q - g.vbase;
    if (ok && j >= 0 && j < g.cnt) {
        const long long num = j * g.n, m = g.cnt;
        const long long i0 = (num / m) % g.n, i1 = (i0 + 1) % g.n;                                         // (j < m: num / m < n already)
        const double t = (double)(num % m) / (double)m, u = 1.0 - (double)g.k / (double)g.R;
        const double dp = (double)g.n * (double)(1 << FILL_POS_BITS), dc = (double)g.n * (double)(1 << FILL_COL_BITS);
        const long long* row = rows + (long long)g.l * SUM_ROW;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double ce = (double)row[a] / dp;
            double y = ce;
            if (g.k < g.R) {
                const double s0 = S[3 * (g.off + i0) + a], s1 = S[3 * (g.off + i1) + a];
                const double s = s0 + t * (s1 - s0);
                y = ce + u * (s - ce);
            }
            x[a] = (float)(fr.centre[a] + y * fr.inv_scale);
            if (colors_out) {
                const double cc = (double)row[6 + a] / dc;
                double z = cc;
                if (g.k < g.R) {
                    const double s0 = SC[3 * (g.off + i0) + a], s1 = SC[3 * (g.off + i1) + a];
                    const double s = s0 + t * (s1 - s0);
                    z = cc + u * (s - cc);
                }
                c[a] = (float)z;
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        vertices_out[3 * (n_old + q) + a] = x[a];
        if (colors_out) colors_out[3 * (n_old + q) + a] = c[a];
    }
}

// signed area of (a, b, c) against N, twice
__device__ __forceinline__ double fill_area(const double (&a)[3], const double (&b)[3], const double (&c)[3], const double (&N)[3]) {
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    double n[3];
    cross3(e1, e2, n);
    return (n[0] * N[0] + n[1] * N[1]) + n[2] * N[2];
}

__global__ __launch_bounds__(FILL_THREADS) void fill_face_kernel(long long n_total, long long n_new_faces, const int* __restrict__ face_ring,
                                                                 long long n_rings, const int* __restrict__ rings, long long n_loops,
                                                                 const long long* __restrict__ loop_offsets, long long n_rim,
                                                                 const int* __restrict__ loop_vertices, const long long* __restrict__ rows,
                                                                 const float* __restrict__ vertices_out, int* __restrict__ faces_out) {
    const long long f = (long long)blockIdx.x * FILL_THREADS + threadIdx.x;
    if (f >= n_new_faces) return;
    int o[3] = {0, 0, 0};
    FillRing g = {};
    const bool ok = fill_ring(rings, n_rings, face_ring[f], loop_offsets, n_loops, n_rim, g);
    const long long e = f - g.fbase;
    if (ok && e >= 0 && e < g.nf) {
        const long long n = g.n, m = g.pcnt, mi = g.cnt;
        // vertex i of the ring outside this strip: the rim (through loop_vertices) or the ring before
        auto prev = [&](long long i) { return g.pbase < 0 ? loop_vertices[g.off + i] : (int)(g.pbase + i); };
        if (n == 3 && g.nf == 1) {
            o[0] = loop_vertices[g.off], o[1] = loop_vertices[g.off + 1], o[2] = loop_vertices[g.off + 2];
        } else if (g.k == g.R) {                                                                            // the fan to the centre
            if (m >= 1 && (g.pbase >= 0 || m == n) && e < m) o[0] = prev(e), o[1] = prev((e + 1) % m), o[2] = g.vbase;
        } else if (g.k == 1) {                                                                              // rim -> ring 1: a quad per rim edge
            const long long i = e >> 1, i1 = (i + 1) % n;
            if (g.pbase < 0 && mi == n && i < n) {
                const int id[4] = {loop_vertices[g.off + i], loop_vertices[g.off + i1], (int)(g.vbase + i1), (int)(g.vbase + i)};   // r0 r1 q1 q0
                if (in_range(id[0], n_total) && in_range(id[1], n_total) && in_range(id[2], n_total) && in_range(id[3], n_total)) {
                    double p[4][3], N[3];
#pragma unroll
                    for (int c = 0; c < 4; ++c)
#pragma unroll
                        for (int a = 0; a < 3; ++a) p[c][a] = (double)vertices_out[3 * (long long)id[c] + a];
#pragma unroll
                    for (int a = 0; a < 3; ++a) N[a] = (double)rows[(long long)g.l * SUM_ROW + 3 + a];
                    const double t1 = fill_area(p[0], p[1], p[2], N), t2 = fill_area(p[0], p[2], p[3], N);          // diagonal r0 - q1
                    const double u1 = fill_area(p[0], p[1], p[3], N), u2 = fill_area(p[1], p[2], p[3], N);          // diagonal r1 - q0
                    const double first = t1 < t2 ? t1 : t2, second = u1 < u2 ? u1 : u2;
                    if (second > first) {
                        if (e & 1) o[0] = id[1], o[1] = id[2], o[2] = id[3];
                        else o[0] = id[0], o[1] = id[1], o[2] = id[3];
                    } else {
                        if (e & 1) o[0] = id[0], o[1] = id[2], o[2] = id[3];
                        else o[0] = id[0], o[1] = id[1], o[2] = id[2];
                    }
                }
            }
        } else if (g.pbase >= 0 && m >= 1 && mi >= 1) {                                                     // ring k - 1 (m) -> ring k (mi): the merge by parameter
            if (e < m) {
                o[0] = (int)(g.pbase + e), o[1] = (int)(g.pbase + (e + 1) % m), o[2] = (int)(g.vbase + (((e + 1) * mi - 1) / m) % mi);
            } else if (e - m < mi) {
                const long long j = e - m;
                o[0] = (int)(g.pbase + (((j + 1) * m) / mi) % m), o[1] = (int)(g.vbase + (j + 1) % mi), o[2] = (int)(g.vbase + j);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) faces_out[3 * f + a] = o[a];
}

}  // namespace
