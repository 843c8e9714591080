// libdgs_mesh_ops.so (include/dgs_mesh_ops.h): TSDF fusion of rendered depth maps, marching tetrahedra, the all-pairs
// nearest-neighbour and closest-triangle searches, the winding-number sums and the earth mover's distance (an auction solver) of the mesh metrics, the
// z-buffer triangle rasterizer of the mesh images, the connected components of the mesh clean-up, the quadric vertex
// clustering of the mesh simplification, the Laplacian / Taubin steps of the mesh smoothing, the quadric edge collapse of the
// mesh decimation and the list ranking and ring emission of the mesh hole filling, gfx950.
// Compiled with -ffp-contract=off: every fp32 operation of the kernels rounds on its own, which is what makes the result equal to
// the PyTorch statement of the same arithmetic (dgs_amd/mesh.py) instead of close to it.
// The kernels live in one header per family (mesh_common.h holds what two families share); this file is the C ABI: the argument
// checks and the launches, one section per family in the order of the includes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <string>

#include "../../include/dgs_mesh_ops.h"
#include "mesh_common.h"
#include "mesh_fusion_kernels.h"
#include "mesh_search_kernels.h"
#include "mesh_raster_kernels.h"
#include "mesh_cc_kernels.h"
#include "mesh_simplify_kernels.h"
#include "mesh_smooth_kernels.h"
#include "mesh_decimate_kernels.h"
#include "mesh_fill_kernels.h"

namespace {
// ---- shared by every family -----------------------------------------------------------------------------------------------------
thread_local std::string g_err;
int fail(int code, const std::string& m) { g_err = m; return code; }

// The status of the launches since the last check, named "<entry>" or "<entry> (<stage>)" in the error.
int launched(const char* entry, const char* stage = nullptr) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    return fail(-2, std::string(entry) + (stage ? " (" + std::string(stage) + ")" : std::string()) + ": " + hipGetErrorString(e));
}

template <class... P, class... A>
int launch(const char* entry, const char* stage, void (*kernel)(P...), dim3 grid, dim3 block, void* stream, A... args) {
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, args...);
    return launched(entry, stage);
}

// The same where a count may be zero: nothing to do is no launch and no error.
template <class... P, class... A>
int launch_if(bool any, const char* entry, const char* stage, void (*kernel)(P...), dim3 grid, dim3 block, void* stream, A... args) {
    return any ? launch(entry, stage, kernel, grid, block, stream, args...) : 0;
}

// Every count in [0, 2^31): ids are int32 (`why` says so), and the fixed-point sums are sized for it.
int check_counts(const char* what, std::initializer_list<long long> counts, const char* why = "ids are int32") {
    for (long long n : counts) {
        if (n < 0) return fail(-1, std::string(what) + ": negative count");
        if (n >= (1LL << 31)) return fail(-1, std::string(what) + ": every count must be below 2^31 (" + why + ")");
    }
    return 0;
}

// A workgroup of 256 threads per 256 items, for a count that passed check_counts: below 2^23 workgroups.
dim3 blocks_of_256(long long n) { return dim3((unsigned)((n + 255) / 256)); }
static_assert(SIMP_THREADS * SIMP_ITEMS_PER_THREAD == 256 && SMOOTH_THREADS == 256 && SMOOTH_VERTS_PER_BLOCK == 256 &&
                  DEC_THREADS * DEC_ITEMS_PER_THREAD == 256 && FILL_THREADS * FILL_ITEMS_PER_THREAD == 256,
              "blocks_of_256 sizes the grids of these families");

// The *_layout entry points: the compile-time sizes of a family, for the wrappers' defaults and the tests' shapes.
template <int N>
int layout(const char* what, int* out, const int (&values)[N]) {
    if (!out) return fail(-1, std::string(what) + ": null pointer");
    for (int i = 0; i < N; ++i) out[i] = values[i];
    return 0;
}

// ---- fusion and marching tetrahedra ---------------------------------------------------------------------------------------------
int check_grid(int Nx, int Ny, int Nz, const char* what) {
    if (Nx < 2 || Ny < 2 || Nz < 2) return fail(-1, std::string(what) + ": every grid dimension must be >= 2");
    return 0;
}

Grid make_grid(int Nx, int Ny, int Nz) { return Grid{Nx, Ny, Nz, (long long)Ny * Nz, (long long)Nz}; }

unsigned blocks_for(long long n, long long cap) {
    long long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ---- the all-pairs searches -----------------------------------------------------------------------------------------------------
// dgs_nn_search, dgs_tri_search and dgs_winding_sum differ by these nouns and sizes and by the kernel they launch; search() is
// everything else.
struct Search {
    const char *what, *empty, *count, *why, *chunk;    // entry point; refusal of an empty set; name of n_*, why it stays below 2^31, name of *_chunk
    int per_block;                                     // queries of a workgroup
    size_t align;                                      // alignment of the set's pointer, bytes
    int fill;                                          // the byte the output starts from: 0xFF under a minimum, 0 under a sum
};
const char* const kLowWordIndex = "the index is the low 32 bits of the packed minimum";
const char* const kLowWordFace = "the face is the low 32 bits of the packed minimum";
const char* const kWindingTerms = "the sum of n_tri terms below 2^30 stays below 2^61";

template <class Launch>
int search(const Search& s, long long n_query, const float* query, long long n_set, const float* set, long long chunk, unsigned long long* best,
           void* stream, Launch launch_kernel) {
    const std::string w = s.what;
    if (n_query < 0) return fail(-1, w + ": negative n_query");
    if (n_set < 1) return fail(-1, w + ": " + s.empty);
    if (n_set >= (1LL << 31)) return fail(-1, w + ": " + s.count + " must be below 2^31 (" + s.why + ")");
    if (chunk < 1) return fail(-1, w + ": " + s.chunk + " must be >= 1");
    if (!set || (n_query > 0 && (!query || !best))) return fail(-1, w + ": null pointer");
    if ((size_t)set % s.align != 0) return fail(-1, w + ": the table must be " + std::to_string(s.align) + "-byte aligned");
    if (n_query == 0) return 0;
    if (chunk > n_set) chunk = n_set;
    const long long slices = (n_set + chunk - 1) / chunk, blocks = (n_query + s.per_block - 1) / s.per_block;
    if (slices > 65535) return fail(-1, w + ": more than 65535 slices: raise " + s.chunk);
    if (blocks > 0x7FFFFFFFLL) return fail(-1, w + ": too many queries for one launch");
    hipError_t e = hipMemsetAsync(best, s.fill, (size_t)n_query * sizeof(unsigned long long), (hipStream_t)stream);
    if (e != hipSuccess) return fail(-2, w + " (init): " + hipGetErrorString(e));
    return launch_kernel(dim3((unsigned)blocks, (unsigned)slices), chunk);
}

// ---- triangle rasterizer --------------------------------------------------------------------------------------------------------
int check_raster(const char* what, int H, int W, long long n_faces, const float* table) {
    if (H < 1 || W < 1) return fail(-1, std::string(what) + ": H and W must be >= 1");
    if ((long long)H * W > (1LL << 30)) return fail(-1, std::string(what) + ": image too large (H * W > 2^30)");
    if (n_faces < 0) return fail(-1, std::string(what) + ": negative n_faces");
    if (n_faces >= (1LL << 31)) return fail(-1, std::string(what) + ": n_faces must be below 2^31 (the face is the low 32 bits of the packed minimum)");
    if (n_faces > 0 && !table) return fail(-1, std::string(what) + ": null pointer");
    if ((size_t)table % 16 != 0) return fail(-1, std::string(what) + ": the table must be 16-byte aligned");
    return 0;
}

// ---- smoothing ------------------------------------------------------------------------------------------------------------------
// The step kernel of dgs_smooth_steps for every channel count C in [1, SMOOTH_MAX_C], at index C - 1.
using SmoothKernel = decltype(&smooth_step_kernel<1>);
const SmoothKernel smooth_kernels[] = {smooth_step_kernel<1>, smooth_step_kernel<2>, smooth_step_kernel<3>, smooth_step_kernel<4>,
                                       smooth_step_kernel<5>, smooth_step_kernel<6>, smooth_step_kernel<7>, smooth_step_kernel<8>};
static_assert(sizeof(smooth_kernels) / sizeof(smooth_kernels[0]) == SMOOTH_MAX_C, "one instantiation per channel count");

// ---- decimation -----------------------------------------------------------------------------------------------------------------
// q_bits in [1, Q_MAX] with n_faces * 2^q_bits <= 2^Q_BUDGET: the overflow bound of include/dgs_mesh_ops.h.
int dec_bits(const char* what, int q_bits, long long n_faces) {
    if (q_bits < 1 || q_bits > DEC_Q_MAX || (n_faces > 0 && n_faces > (1LL << (DEC_Q_BUDGET - q_bits))))
        return fail(-1, std::string(what) + ": q_bits must be in [1, " + std::to_string(DEC_Q_MAX) + "] with n_faces * 2^q_bits <= 2^" +
                            std::to_string(DEC_Q_BUDGET) + " (the quadric sums could overflow)");
    return 0;
}

// ---- hole filling ---------------------------------------------------------------------------------------------------------------
// The frame of dgs_fill_rim and dgs_fill_emit: positions enter the sums as (v - centre) * scale, scale a power of two.
int fill_frame(const char* what, double cx, double cy, double cz, double scale, FillFrame& fr) {
    if (!std::isfinite(cx) || !std::isfinite(cy) || !std::isfinite(cz) || !(scale > 0.0) || !std::isfinite(scale) || !std::isfinite(1.0 / scale))
        return fail(-1, std::string(what) + ": the frame's centre must be finite and its scale positive and finite");
    fr = FillFrame{{cx, cy, cz}, scale, 1.0 / scale};
    return 0;
}
}  // namespace

extern "C" {

int dgs_mesh_ops_abi_version(void) { return DGS_MESH_OPS_ABI_VERSION; }
const char* dgs_mesh_ops_last_error(void) { return g_err.c_str(); }

// ---- fusion and marching tetrahedra (mesh_fusion_kernels.h) ----------------------------------------------------------------------
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
    return launch("dgs_tsdf_integrate", nullptr, tsdf_integrate_kernel, grid, dim3(BZ, BY, 1), stream, Nx, Ny, Nz, ox, oy, oz, voxel, V, H, W, depth,
                  rgb, proj, trunc, depth_trunc, prior_weight, accumulate, tsdf, weight, color);
}

int dgs_mt_classify(int Nx, int Ny, int Nz, const float* tsdf, const float* weight, int* cell_tris, int* point_verts,
                    unsigned char* point_mask, void* stream) {
    const char* w = "dgs_mt_classify";
    if (int rc = check_grid(Nx, Ny, Nz, w)) return rc;
    if (!tsdf || !weight || !cell_tris || !point_verts || !point_mask) return fail(-1, "dgs_mt_classify: null pointer");
    const Grid g = make_grid(Nx, Ny, Nz);
    const long long n = (long long)Nx * Ny * Nz;
    const dim3 grid(blocks_for(n, 1 << 20));
    if (int rc = launch(w, "cells", mt_cells_kernel, grid, dim3(256), stream, g, n, tsdf, weight, cell_tris)) return rc;
    return launch(w, "points", mt_points_kernel, grid, dim3(256), stream, g, n, tsdf, cell_tris, point_verts, point_mask);
}

int dgs_mt_emit(int Nx, int Ny, int Nz, float ox, float oy, float oz, float voxel, const float* tsdf, const float* color, long long n_cells,
                const long long* cells, const int* cell_tris, const long long* tri_incl, long long n_points, const long long* points,
                const unsigned char* point_mask, const long long* vert_incl, float* vertices, float* vertex_colors, int* faces, void* stream) {
    const char* w = "dgs_mt_emit";
    if (int rc = check_grid(Nx, Ny, Nz, w)) return rc;
    if (n_cells < 0 || n_points < 0) return fail(-1, "dgs_mt_emit: negative count");
    if (n_cells == 0 || n_points == 0) return 0;
    if (!tsdf || !cells || !cell_tris || !tri_incl || !points || !point_mask || !vert_incl || !vertices || !faces || (color && !vertex_colors))
        return fail(-1, "dgs_mt_emit: null pointer");
    const Grid g = make_grid(Nx, Ny, Nz);
    if (int rc = launch(w, "vertices", mt_vertices_kernel, dim3(blocks_for(n_points, 1LL << 31)), dim3(256), stream, g, ox, oy, oz, voxel, tsdf, color,
                        n_points, points, point_mask, vert_incl, vertices, vertex_colors))
        return rc;
    return launch(w, "faces", mt_faces_kernel, dim3(blocks_for(n_cells, 1LL << 31)), dim3(256), stream, g, tsdf, n_cells, cells, cell_tris, tri_incl,
                  point_mask, vert_incl, faces);
}

// ---- the searches, the winding sums and the earth mover's distance (mesh_search_kernels.h) -----------------------------------------------------
int dgs_nn_search(long long n_query, const float* query, long long n_ref, const float* ref, long long ref_chunk, unsigned long long* best,
                  void* stream) {
    const Search s{"dgs_nn_search", "the reference set must hold at least one point (n_ref >= 1)", "n_ref", kLowWordIndex, "ref_chunk", NN_Q, 1, 0xFF};
    return search(s, n_query, query, n_ref, ref, ref_chunk, best, stream, [&](dim3 grid, long long chunk) {
        return launch(s.what, nullptr, nn_search_kernel, grid, dim3(NN_THREADS), stream, n_query, query, n_ref, ref, chunk, best);
    });
}

int dgs_nn_layout(int out[3]) { return layout("dgs_nn_layout", out, {NN_Q, NN_T, NN_CHUNK}); }

int dgs_tri_search(long long n_query, const float* query, long long n_tri, const float* table, long long tri_chunk, unsigned long long* best,
                   void* stream) {
    const Search s{"dgs_tri_search", "the table must hold at least one triangle (n_tri >= 1)", "n_tri", kLowWordFace, "tri_chunk", TRI_Q, 16, 0xFF};
    return search(s, n_query, query, n_tri, table, tri_chunk, best, stream, [&](dim3 grid, long long chunk) {
        return launch(s.what, nullptr, tri_search_kernel, grid, dim3(TRI_THREADS), stream, n_query, query, n_tri,
                      reinterpret_cast<const float4*>(table), chunk, best);
    });
}

int dgs_tri_layout(int out[4]) { return layout("dgs_tri_layout", out, {TRI_Q, TRI_T, TRI_CHUNK, TRI_ROW}); }

int dgs_winding_sum(long long n_query, const float* query, long long n_tri, const float* table, long long tri_chunk, long long* sums,
                    void* stream) {
    const Search s{"dgs_winding_sum", "the table must hold at least one triangle (n_tri >= 1)", "n_tri", kWindingTerms, "tri_chunk", WIND_Q, 16, 0};
    unsigned long long* out = reinterpret_cast<unsigned long long*>(sums);
    return search(s, n_query, query, n_tri, table, tri_chunk, out, stream, [&](dim3 grid, long long chunk) {
        return launch(s.what, nullptr, winding_sum_kernel, grid, dim3(WIND_THREADS), stream, n_query, query, n_tri,
                      reinterpret_cast<const float4*>(table), chunk, out);
    });
}

int dgs_winding_layout(int out[4]) { return layout("dgs_winding_layout", out, {WIND_Q, WIND_T, WIND_CHUNK, WIND_ROW}); }

int dgs_emd_auction(long long n, const float* a, const float* b, float inv_q, long long max_rounds, void* scratch, long long scratch_bytes,
                    int* assignment, long long* prices, long long* result, void* stream) {
    const std::string w = "dgs_emd_auction";
    if (!result) return fail(-1, w + ": null pointer (result)");
    for (int k = 0; k < EMD_RESULTS; ++k) result[k] = 0;
    if (n < 0) return fail(-1, w + ": negative n");
    if (n >= (1LL << EMD_BIDDER_BITS)) return fail(-1, w + ": n must be below 2^24 (the bidder is the low 24 bits of the packed bid)");
    if (max_rounds <= 0) return fail(-1, w + ": max_rounds must be >= 1");
    if (!(inv_q >= 0.0f) || inv_q > 3.0e38f) return fail(-1, w + ": inv_q must be finite and >= 0");
    if (n == 0) return 0;
    if (!a || !b || !assignment || !prices) return fail(-1, w + ": null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    auto hip_failed = [&](const char* what) { return fail(-2, w + " (" + what + "): " + hipGetErrorString(e)); };
    if (n == 1) {                                                          // no second best: the trivial matching, nothing launched
        float pa[3], pb[3];
        if ((e = hipMemcpyAsync(pa, a, sizeof pa, hipMemcpyDeviceToHost, st)) != hipSuccess) return hip_failed("read a");
        if ((e = hipMemcpyAsync(pb, b, sizeof pb, hipMemcpyDeviceToHost, st)) != hipSuccess) return hip_failed("read b");
        if ((e = hipMemsetAsync(assignment, 0, sizeof(int), st)) != hipSuccess) return hip_failed("assignment");
        if ((e = hipMemsetAsync(prices, 0, sizeof(long long), st)) != hipSuccess) return hip_failed("prices");
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_failed("synchronise");
        const float dx = pa[0] - pb[0], dy = pa[1] - pb[1], dz = pa[2] - pb[2];   // emd_cost on the host (this file is built with
        const float d = std::sqrt((dx * dx + dy * dy) + dz * dz);                 // -ffp-contract=off for the host too)
        result[0] = result[1] = (long long)std::fmin(std::nearbyint(d * inv_q), EMD_COST_CAP);
        return 0;
    }
    if (!scratch) return fail(-1, w + ": null pointer (scratch)");
    if ((size_t)scratch % 8 != 0) return fail(-1, w + ": the scratch buffer must be 8-byte aligned");
    if (scratch_bytes < EMD_SCRATCH_FIXED + n * EMD_SCRATCH_PER_POINT)
        return fail(-1, w + ": the scratch buffer is too small (" + std::to_string(EMD_SCRATCH_FIXED) + " + " + std::to_string(EMD_SCRATCH_PER_POINT) +
                            " bytes per point are needed, dgs_emd_layout)");
    // scratch: control block | word [n] u64 | mine [n] u64 | owner, target, list0, list1 [n] int32 each
    EmdState s;
    s.n = (int)n, s.inv_q = inv_q, s.a = a, s.b = b, s.price = prices, s.assign = assignment;
    s.ctrl = reinterpret_cast<EmdCtrl*>(scratch);
    s.word = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(scratch) + EMD_SCRATCH_FIXED);
    s.mine = s.word + n;
    s.owner = reinterpret_cast<int*>(s.mine + n), s.target = s.owner + n, s.list0 = s.target + n, s.list1 = s.list0 + n;
    EmdCtrl h;
    auto read_ctrl = [&]() {
        if ((e = hipMemcpyAsync(&h, s.ctrl, sizeof h, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        return e = hipStreamSynchronize(st);
    };
    // the control block and the words start at 0 (the two are adjacent), the prices too
    if ((e = hipMemsetAsync(scratch, 0, EMD_SCRATCH_FIXED + (size_t)n * sizeof(unsigned long long), st)) != hipSuccess) return hip_failed("init");
    if ((e = hipMemsetAsync(prices, 0, (size_t)n * sizeof(long long), st)) != hipSuccess) return hip_failed("init");
    const dim3 threads(EMD_THREADS);
    const unsigned per_point = (unsigned)((n + EMD_THREADS - 1) / EMD_THREADS);
    const unsigned per_wave = (unsigned)std::min<long long>((n + EMD_WAVES - 1) / EMD_WAVES, EMD_MAX_BLOCKS);
    if (int rc = launch("dgs_emd_auction", "max cost", emd_max_cost_kernel, dim3(per_wave), threads, stream, s)) return rc;
    if (read_ctrl() != hipSuccess) return hip_failed("max cost");
    long long eps = std::max<long long>(1, h.max_cost / 2), rounds = 0;
    int phase = 0;
    for (;; ++phase) {
        hipLaunchKernelGGL(emd_phase_kernel, dim3(per_point), threads, 0, st, s);
        long long bidders = n;                                             // an upper bound for the whole phase: the count never grows
        for (int cur = 0; bidders > 0;) {
            const long long left = max_rounds - rounds;
            if (left <= 0) {
                result[2] = rounds, result[3] = h.max_cost, result[4] = phase, result[5] = eps, result[6] = bidders;
                return fail(-3, w + ": max_rounds = " + std::to_string(max_rounds) + " reached in phase " + std::to_string(phase) + " (eps " +
                                    std::to_string(eps) + ") with " + std::to_string(bidders) + " of " + std::to_string(n) + " still unassigned");
            }
            const bool dense = bidders > EMD_SPARSE_MAX;
            const long long batch = std::min<long long>(left, dense ? EMD_DENSE_BATCH : EMD_SPARSE_BATCH);
            const dim3 bid_grid((unsigned)(dense ? (bidders + EMD_THREADS - 1) / EMD_THREADS : bidders));   // sparse: a workgroup per bidder
            const dim3 resolve_grid((unsigned)((bidders + EMD_THREADS - 1) / EMD_THREADS));
            for (long long r = 0; r < batch; ++r, cur ^= 1) {              // rounds after the phase has converged are no-ops
                if (dense)
                    hipLaunchKernelGGL(emd_bid_dense_kernel, bid_grid, threads, 0, st, s, cur, eps);
                else
                    hipLaunchKernelGGL(emd_bid_sparse_kernel, bid_grid, threads, 0, st, s, cur, eps);
                hipLaunchKernelGGL(emd_resolve_kernel, resolve_grid, threads, 0, st, s, cur);
            }
            if (int rc = launched("dgs_emd_auction", "round")) return rc;
            if (read_ctrl() != hipSuccess) return hip_failed("round");
            if (h.status != 0) return fail(-4, w + ": a bid of phase " + std::to_string(phase) + " does not fit 39 bits");
            bidders = h.count[cur], rounds = h.rounds;
        }
        if (eps == 1) break;
        eps = std::max<long long>(1, eps / 4);
    }
    if ((e = hipMemsetAsync(assignment, 0xFF, (size_t)n * sizeof(int), st)) != hipSuccess) return hip_failed("assignment");
    hipLaunchKernelGGL(emd_assign_kernel, dim3(per_point), threads, 0, st, s);
    if (int rc = launch("dgs_emd_auction", "sums", emd_sums_kernel, dim3(per_wave), threads, stream, s)) return rc;
    if (read_ctrl() != hipSuccess) return hip_failed("sums");
    if (h.status != 0) return fail(-5, w + ": the owners are not a permutation at the end");
    result[0] = h.primal, result[1] = h.sum_min - h.sum_price, result[2] = h.rounds, result[3] = h.max_cost, result[4] = phase + 1, result[5] = eps;
    return 0;
}

int dgs_emd_layout(int out[6]) {
    return layout("dgs_emd_layout", out, {EMD_THREADS, EMD_T, EMD_SPARSE_MAX, EMD_RESULTS, EMD_SCRATCH_FIXED, EMD_SCRATCH_PER_POINT});
}

// ---- triangle rasterizer (mesh_raster_kernels.h) ---------------------------------------------------------------------------------
int dgs_mesh_raster(long long n_faces, const float* table, const int* list, long long n_list, int path, int H, int W,
                    unsigned long long* best, int clear, void* stream) {
    const char* w = "dgs_mesh_raster";
    if (int rc = check_raster(w, H, W, n_faces, table)) return rc;
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
    if (path == 0)
        return launch(w, "small", raster_small_kernel, dim3((unsigned)((n_list + RAS_THREADS - 1) / RAS_THREADS)), dim3(RAS_THREADS), stream, n_faces, rows,
                      list, n_list, H, W, best);
    // few large faces: several workgroups per face, each a stripe of its rows; many: one each.  The result does not depend on it.
    long long stripes = RAS_TARGET_GROUPS / n_list, rows_of_tiles = ((long long)H + RAS_TILE_Y - 1) / RAS_TILE_Y;
    stripes = stripes < 1 ? 1 : (stripes > RAS_MAX_STRIPES ? RAS_MAX_STRIPES : stripes);
    if (stripes > rows_of_tiles) stripes = rows_of_tiles;
    // (a launch of 2^32 threads or more along x is refused: above RAS_MAX_GROUPS faces a workgroup takes several of them in turn)
    const long long groups = n_list < RAS_MAX_GROUPS ? n_list : RAS_MAX_GROUPS;
    return launch(w, "large", raster_large_kernel, dim3((unsigned)groups, (unsigned)stripes), dim3(RAS_THREADS), stream, n_faces, rows, list, n_list, H,
                  W, best);
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
    return launch("dgs_mesh_resolve", nullptr, raster_resolve_kernel, dim3((unsigned)((n + RAS_THREADS - 1) / RAS_THREADS)), dim3(RAS_THREADS), stream, H, W,
                  best, n_faces, reinterpret_cast<const float4*>(table), faces, n_vertices, attr, C, background, face_id, depth, bary,
                  C > 0 ? image : nullptr);
}

int dgs_mesh_raster_layout(int out[4]) { return layout("dgs_mesh_raster_layout", out, {RAS_SMALL_AREA, RAS_THREADS, RAS_ROW, RAS_MAX_C}); }

// ---- connected components (mesh_cc_kernels.h) ------------------------------------------------------------------------------------
int dgs_cc_labels(long long n_nodes, const int* groups, long long n_groups, int k, int* label, void* stream) {
    const char* w = "dgs_cc_labels";
    if (k != 2 && k != 3) return fail(-1, "dgs_cc_labels: k must be 2 or 3");
    if (n_nodes < 0 || n_groups < 0) return fail(-1, "dgs_cc_labels: negative count");
    if (n_nodes >= (1LL << 31)) return fail(-1, "dgs_cc_labels: n_nodes must be below 2^31 (labels are int32)");
    if ((n_nodes > 0 && !label) || (n_groups > 0 && !groups)) return fail(-1, "dgs_cc_labels: null pointer");
    if (n_nodes == 0) return 0;
    const long long per_block = (long long)CC_THREADS * CC_GROUPS_PER_THREAD;
    auto blocks = [&](long long n) { const long long b = (n + per_block - 1) / per_block; return dim3((unsigned)(b > CC_MAX_BLOCKS ? CC_MAX_BLOCKS : b)); };
    if (int rc = launch(w, "init", cc_init_kernel, blocks(n_nodes), dim3(CC_THREADS), stream, n_nodes, label)) return rc;
    if (n_groups == 0) return 0;
    decltype(&cc_hook_kernel<2>) hook = cc_hook_kernel<2>;
    if (k == 3) hook = cc_hook_kernel<3>;
    if (int rc = launch(w, "hook", hook, blocks(n_groups), dim3(CC_THREADS), stream, n_nodes, groups, n_groups, label)) return rc;
    return launch(w, "compress", cc_compress_kernel, blocks(n_nodes), dim3(CC_THREADS), stream, n_nodes, label);
}

int dgs_cc_layout(int out[2]) { return layout("dgs_cc_layout", out, {CC_THREADS, CC_GROUPS_PER_THREAD}); }

// ---- simplification (mesh_simplify_kernels.h) ------------------------------------------------------------------------------------
int dgs_simplify_accumulate(long long n_vertices, const float* vertices, const float* colors, long long n_faces, const int* faces,
                            const int* cluster, long long n_clusters, const float* centres, float cell, long long* rows, void* stream) {
    const char* w = "dgs_simplify_accumulate";
    if (int rc = check_counts(w, {n_vertices, n_faces, n_clusters}, "ids are int32, and the sums are sized for it")) return rc;
    if (!(cell > 0.0f) || !std::isfinite(cell)) return fail(-1, "dgs_simplify_accumulate: cell must be positive and finite");
    if ((n_clusters > 0 && (!rows || !centres)) || (n_vertices > 0 && (!vertices || !cluster)) || (n_faces > 0 && (!faces || !vertices || !cluster)))
        return fail(-1, "dgs_simplify_accumulate: null pointer");
    if (n_clusters == 0) return 0;
    hipError_t e = hipMemsetAsync(rows, 0, (size_t)n_clusters * SUM_ROW * sizeof(long long), (hipStream_t)stream);
    if (e != hipSuccess) return fail(-2, std::string("dgs_simplify_accumulate (clear): ") + hipGetErrorString(e));
    if (int rc = launch_if(n_vertices > 0, w, "vertices", simp_vertex_kernel, blocks_of_256(n_vertices), dim3(SIMP_THREADS), stream, n_vertices,
                           vertices, colors, cluster, n_clusters, centres, cell, rows))
        return rc;
    return launch_if(n_faces > 0 && n_vertices > 0, w, "faces", simp_face_kernel, blocks_of_256(n_faces), dim3(SIMP_THREADS), stream, n_faces,
                     faces, n_vertices, vertices, cluster, n_clusters, centres, cell, rows);
}

int dgs_simplify_solve(long long n_clusters, const long long* rows, const float* centres, float cell, int placement, float* vertices,
                       float* colors, void* stream) {
    if (n_clusters < 0) return fail(-1, "dgs_simplify_solve: negative count");
    if (n_clusters >= (1LL << 31)) return fail(-1, "dgs_simplify_solve: n_clusters must be below 2^31");
    if (placement != 0 && placement != 1) return fail(-1, "dgs_simplify_solve: placement must be 0 (average) or 1 (quadric)");
    if (!(cell > 0.0f) || !std::isfinite(cell)) return fail(-1, "dgs_simplify_solve: cell must be positive and finite");
    if (n_clusters > 0 && (!rows || !centres || !vertices)) return fail(-1, "dgs_simplify_solve: null pointer");
    if (n_clusters == 0) return 0;
    return launch("dgs_simplify_solve", nullptr, simp_solve_kernel, blocks_of_256(n_clusters), dim3(SIMP_THREADS), stream, n_clusters, rows, centres, cell,
                  placement, vertices, colors);
}

int dgs_simplify_layout(int out[5]) {
    return layout("dgs_simplify_layout", out, {SIMP_THREADS, SIMP_ITEMS_PER_THREAD, SIMP_Q, SIMP_W_MAX, SIMP_LAMBDA_EXP});
}

// ---- smoothing (mesh_smooth_kernels.h) -------------------------------------------------------------------------------------------
int dgs_smooth_steps(long long n_vertices, const long long* offsets, const int* neighbours, long long n_entries, int C, int mode,
                     const float* factors, int n_steps, const unsigned char* pinned, float* x, float* tmp, void* stream) {
    if (int rc = check_counts("dgs_smooth_steps", {n_vertices, n_entries, n_steps})) return rc;
    if (C < 1 || C > SMOOTH_MAX_C) return fail(-1, "dgs_smooth_steps: C must be in [1, " + std::to_string(SMOOTH_MAX_C) + "]");
    if (mode != 0 && mode != 1) return fail(-1, "dgs_smooth_steps: mode must be 0 (laplacian) or 1 (simple)");
    if (n_steps > SMOOTH_MAX_STEPS) return fail(-1, "dgs_smooth_steps: n_steps must be at most " + std::to_string(SMOOTH_MAX_STEPS) + " (dgs_smooth_layout)");
    if ((n_steps > 0 && !factors) || (n_vertices > 0 && (!offsets || !x || !tmp)) || (n_entries > 0 && !neighbours))
        return fail(-1, "dgs_smooth_steps: null pointer");
    for (int k = 0; k < n_steps; ++k)
        if (!std::isfinite(factors[k])) return fail(-1, "dgs_smooth_steps: factor " + std::to_string(k) + " is not finite");
    if (n_steps == 0 || n_vertices == 0) return 0;
    const SmoothKernel kernel = smooth_kernels[C - 1];
    float *src = x, *dst = tmp;
    for (int k = 0; k < n_steps; ++k) {
        if (int rc = launch("dgs_smooth_steps", nullptr, kernel, blocks_of_256(n_vertices), dim3(SMOOTH_THREADS), stream, n_vertices, offsets, neighbours,
                            n_entries, mode, factors[k], pinned, src, dst))
            return rc;
        std::swap(src, dst);
    }
    if (src != x) {                                                        // an odd count left the result in tmp
        hipError_t e = hipMemcpyAsync(x, tmp, (size_t)n_vertices * C * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return fail(-2, std::string("dgs_smooth_steps (copy): ") + hipGetErrorString(e));
    }
    return 0;
}

int dgs_smooth_layout(int out[4]) {
    return layout("dgs_smooth_layout", out, {SMOOTH_THREADS, SMOOTH_VERTS_PER_BLOCK, SMOOTH_MAX_C, SMOOTH_MAX_STEPS});
}

// ---- decimation (mesh_decimate_kernels.h) ----------------------------------------------------------------------------------------
int dgs_decimate_quadrics(long long n_vertices, const float* pos, long long n_faces, const int* faces, float mean_len, int q_bits,
                          long long* rows, void* stream) {
    const char* w = "dgs_decimate_quadrics";
    if (int rc = check_counts(w, {n_vertices, n_faces})) return rc;
    if (int rc = dec_bits(w, q_bits, n_faces)) return rc;
    if (!(mean_len > 0.0f) || !std::isfinite(mean_len)) return fail(-1, "dgs_decimate_quadrics: mean_len must be positive and finite");
    if ((n_vertices > 0 && (!pos || !rows)) || (n_faces > 0 && !faces)) return fail(-1, "dgs_decimate_quadrics: null pointer");
    if (n_vertices == 0) return 0;
    hipError_t e = hipMemsetAsync(rows, 0, (size_t)n_vertices * DEC_ROW * sizeof(long long), (hipStream_t)stream);
    if (e != hipSuccess) return fail(-2, std::string("dgs_decimate_quadrics (clear): ") + hipGetErrorString(e));
    if (n_faces == 0) return 0;
    return launch(w, nullptr, dec_quadric_kernel, blocks_of_256(n_faces), dim3(DEC_THREADS), stream, n_faces, faces, n_vertices, pos, mean_len,
                  std::ldexp(1.0, q_bits), rows);
}

int dgs_decimate_edges(long long n_vertices, const float* pos, const long long* rows, const unsigned char* flags, long long n_faces,
                       const int* faces, long long n_edges, const int* edges, const long long* adj_offsets, const int* adj, long long n_adj,
                       const long long* vf_offsets, const int* vf, long long n_vf, int q_bits, float max_cost, float* cost, float* place,
                       unsigned char* valid, void* stream) {
    const char* w = "dgs_decimate_edges";
    if (int rc = check_counts(w, {n_vertices, n_faces, n_edges, n_adj, n_vf})) return rc;
    if (int rc = dec_bits(w, q_bits, n_faces)) return rc;
    if (!(max_cost >= 0.0f)) return fail(-1, "dgs_decimate_edges: max_cost must be >= 0 (+inf for no bound)");
    if ((n_vertices > 0 && (!pos || !rows || !flags || !adj_offsets || !vf_offsets)) || (n_faces > 0 && !faces) || (n_adj > 0 && !adj) ||
        (n_vf > 0 && !vf) || (n_edges > 0 && (!edges || !cost || !place || !valid)))
        return fail(-1, "dgs_decimate_edges: null pointer");
    if (n_edges == 0) return 0;
    return launch(w, nullptr, dec_edge_kernel, blocks_of_256(n_edges), dim3(DEC_THREADS), stream, n_vertices, pos, rows, flags, n_faces, faces, n_edges,
                  edges, adj_offsets, adj, n_adj, vf_offsets, vf, n_vf, std::ldexp(1.0, -q_bits), max_cost, cost, place, valid);
}

int dgs_decimate_select(long long n_vertices, long long n_edges, const int* edges, const float* cost, const unsigned char* compete,
                        unsigned long long* m1, unsigned long long* m2, unsigned char* selected, void* stream) {
    const char* w = "dgs_decimate_select";
    if (int rc = check_counts(w, {n_vertices, n_edges})) return rc;
    if ((n_vertices > 0 && (!m1 || !m2)) || (n_edges > 0 && (!edges || !cost || !compete || !selected))) return fail(-1, "dgs_decimate_select: null pointer");
    const dim3 per_vertex = blocks_of_256(n_vertices), per_edge = blocks_of_256(n_edges), threads(DEC_THREADS);
    if (int rc = launch_if(n_vertices > 0, w, "init", dec_fill_kernel, per_vertex, threads, stream, n_vertices, m1, DEC_NO_KEY)) return rc;
    if (int rc = launch_if(n_edges > 0 && n_vertices > 0, w, "pass 1", dec_select_kernel<1>, per_edge, threads, stream, n_vertices, n_edges, edges,
                           cost, compete, m1, m2, selected))
        return rc;
    if (n_vertices > 0) {
        hipError_t e = hipMemcpyAsync(m2, m1, (size_t)n_vertices * sizeof(unsigned long long), hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return fail(-2, std::string("dgs_decimate_select (copy): ") + hipGetErrorString(e));
    }
    if (n_edges == 0) return 0;
    if (int rc = launch_if(n_vertices > 0, w, "pass 2", dec_select_kernel<2>, per_edge, threads, stream, n_vertices, n_edges, edges, cost, compete, m1,
                           m2, selected))
        return rc;
    return launch(w, "pass 3", dec_select_kernel<3>, per_edge, threads, stream, n_vertices, n_edges, edges, cost, compete, m1, m2, selected);
}

int dgs_decimate_apply(long long n_vertices, float* pos, long long* rows, float* colors, const unsigned char* flags, unsigned char* moved, int* vmap,
                       long long n_edges, const int* edges, const float* place, long long n_sel, const int* sel, long long n_faces, int* faces,
                       unsigned char* keep, void* stream) {
    const char* w = "dgs_decimate_apply";
    if (int rc = check_counts(w, {n_vertices, n_edges, n_sel, n_faces})) return rc;
    if ((n_vertices > 0 && (!pos || !rows || !flags || !moved || !vmap)) || (n_edges > 0 && (!edges || !place)) || (n_sel > 0 && !sel) ||
        (n_faces > 0 && (!faces || !keep)))
        return fail(-1, "dgs_decimate_apply: null pointer");
    const dim3 threads(DEC_THREADS);
    if (int rc = launch_if(n_vertices > 0, w, "init", dec_iota_kernel, blocks_of_256(n_vertices), threads, stream, n_vertices, vmap)) return rc;
    if (int rc = launch_if(n_sel > 0 && n_edges > 0 && n_vertices > 0, w, "collapse", dec_collapse_kernel, blocks_of_256(n_sel), threads, stream,
                           n_vertices, pos, rows, colors, flags, moved, vmap, n_edges, edges, place, n_sel, sel))
        return rc;
    return launch_if(n_faces > 0, w, "faces", dec_reindex_kernel, blocks_of_256(n_faces), threads, stream, n_faces, faces, n_vertices, vmap,
                     keep);
}

int dgs_decimate_layout(int out[8]) {
    return layout("dgs_decimate_layout", out, {DEC_THREADS, DEC_ITEMS_PER_THREAD, DEC_Q_MAX, DEC_Q_BUDGET, DEC_W_MAX, DEC_LAMBDA_EXP, DEC_MIN_VALENCE,
                                               DEC_LEN_BITS});
}

// ---- hole filling (mesh_fill_kernels.h) ------------------------------------------------------------------------------------------
int dgs_fill_rank(long long n_nodes, const int* succ, const int* leader, int n_rounds, unsigned long long* buf_a, unsigned long long* buf_b,
                  int* rank, void* stream) {
    const char* w = "dgs_fill_rank";
    if (int rc = check_counts(w, {n_nodes})) return rc;
    if (n_rounds < 0 || n_rounds > FILL_MAX_ROUNDS)
        return fail(-1, "dgs_fill_rank: n_rounds must be in [0, " + std::to_string(FILL_MAX_ROUNDS) + "] (2^n_rounds nodes are the longest list)");
    if (n_nodes > 0 && (!succ || !leader || !buf_a || !buf_b || !rank)) return fail(-1, "dgs_fill_rank: null pointer");
    if (n_nodes > 0 && buf_a == buf_b) return fail(-1, "dgs_fill_rank: buf_a and buf_b must be two buffers (a round reads one and writes the other)");
    if (n_nodes == 0) return 0;
    const dim3 grid = blocks_of_256(n_nodes), threads(FILL_THREADS);
    if (int rc = launch(w, "init", fill_rank_init_kernel, grid, threads, stream, n_nodes, succ, leader, buf_a)) return rc;
    unsigned long long *in = buf_a, *out = buf_b;
    for (int r = 0; r < n_rounds; ++r) {
        if (int rc = launch(w, "round", fill_rank_round_kernel, grid, threads, stream, n_nodes, in, out)) return rc;
        std::swap(in, out);
    }
    return launch(w, "ranks", fill_rank_final_kernel, grid, threads, stream, n_nodes, leader, in, rank);
}

int dgs_fill_rim(long long n_vertices, const float* vertices, const float* colors, long long n_rim, const int* loop_vertices, const int* rim_loop,
                 long long n_loops, const long long* loop_offsets, double centre_x, double centre_y, double centre_z, double scale, double* S,
                 double* SC, long long* rows, void* stream) {
    const char* w = "dgs_fill_rim";
    if (int rc = check_counts(w, {n_vertices, n_rim, n_loops})) return rc;
    FillFrame fr;
    if (int rc = fill_frame(w, centre_x, centre_y, centre_z, scale, fr)) return rc;
    if ((n_vertices > 0 && !vertices) || (n_rim > 0 && (!loop_vertices || !rim_loop || !S)) || (n_loops > 0 && (!loop_offsets || !rows)) ||
        (n_rim > 0 && (colors != nullptr) != (SC != nullptr)))
        return fail(-1, "dgs_fill_rim: null pointer (colors and SC come together)");
    if (n_loops == 0) return 0;
    hipError_t e = hipMemsetAsync(rows, 0, (size_t)n_loops * SUM_ROW * sizeof(long long), (hipStream_t)stream);
    if (e != hipSuccess) return fail(-2, std::string("dgs_fill_rim (clear): ") + hipGetErrorString(e));
    if (n_rim == 0) return 0;
    return launch(w, nullptr, fill_rim_kernel, blocks_of_256(n_rim), dim3(FILL_THREADS), stream, n_vertices, vertices, colors, n_rim, loop_vertices, rim_loop,
                  n_loops, loop_offsets, fr, S, SC, rows);
}

int dgs_fill_emit(long long n_old, long long n_new, const int* vert_ring, long long n_new_faces, const int* face_ring, long long n_rings,
                  const int* rings, long long n_loops, const long long* loop_offsets, long long n_rim, const int* loop_vertices,
                  const long long* rows, const double* S, const double* SC, double centre_x, double centre_y, double centre_z, double scale,
                  float* vertices_out, float* colors_out, int* faces_out, void* stream) {
    const char* w = "dgs_fill_emit";
    if (int rc = check_counts(w, {n_old, n_new, n_old + n_new, n_new_faces, n_rings, n_loops, n_rim})) return rc;
    FillFrame fr;
    if (int rc = fill_frame(w, centre_x, centre_y, centre_z, scale, fr)) return rc;
    const bool any = n_new > 0 || n_new_faces > 0;
    if ((n_new > 0 && !vert_ring) || (n_new_faces > 0 && (!face_ring || !faces_out)) || (n_old + n_new > 0 && any && !vertices_out) ||
        (any && (!rings || !loop_offsets || !loop_vertices || !rows || !S)) || (n_new > 0 && (colors_out != nullptr) != (SC != nullptr)))
        return fail(-1, "dgs_fill_emit: null pointer (colors_out and SC come together)");
    if (any && (n_rings == 0 || n_loops == 0 || n_rim == 0)) return fail(-1, "dgs_fill_emit: new vertices or faces without rings, loops or a rim");
    if (int rc = launch_if(n_new > 0, w, "vertices", fill_vertex_kernel, blocks_of_256(n_new), dim3(FILL_THREADS), stream, n_old, n_new, vert_ring,
                           n_rings, rings, n_loops, loop_offsets, n_rim, rows, S, SC, fr, vertices_out, colors_out))
        return rc;
    return launch_if(n_new_faces > 0, w, "faces", fill_face_kernel, blocks_of_256(n_new_faces), dim3(FILL_THREADS), stream, n_old + n_new,
                     n_new_faces, face_ring, n_rings, rings, n_loops, loop_offsets, n_rim, loop_vertices, rows, vertices_out,
                     faces_out);
}

int dgs_fill_layout(int out[8]) {
    return layout("dgs_fill_layout", out, {FILL_THREADS, FILL_ITEMS_PER_THREAD, FILL_POS_BITS, FILL_NRM_BITS, FILL_COL_BITS, FILL_RING_COLS,
                                           FILL_TAPS, FILL_MAX_ROUNDS});
}

}  // extern "C"
