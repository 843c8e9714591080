/*
 * dgs_mesh_ops.h -- C ABI of the mesh kernels: depth-map fusion into a truncated signed distance volume, marching tetrahedra over
 * it, the all-pairs nearest-neighbour and closest-triangle searches behind the geometry metrics of dgs_amd/mesh_metrics.py, the
 * z-buffer triangle rasterizer behind the mesh images of dgs_amd/mesh_render.py, the connected components behind
 * dgs_amd/mesh_clean.py, the quadric vertex clustering behind dgs_amd/mesh_simplify.py, the Laplacian / Taubin steps behind dgs_amd/mesh_smooth.py, and the
 * quadric edge collapse behind dgs_amd/mesh_decimate.py and the loop ranking and ring fill behind dgs_amd/mesh_fill.py.  The first two replace the PyTorch / open3d path of the reference's render_mesh.py:
 *
 *   dgs_tsdf_integrate          <-  utils/mesh_utils.py:218-266  compute_sdf_perframe + compute_unbounded_tsdf (inv_contraction=None)
 *   dgs_mt_classify / _emit     <-  utils/mesh_utils.py:158-199 / :268-271  volume.extract_triangle_mesh() / marching_cubes_with_contraction
 *
 * All pointers are device pointers, fp32 contiguous unless noted; every call is asynchronous on `stream`.
 * Return value: 0 or a negative status, message through dgs_mesh_ops_last_error().
 *
 * THE GRID.  Dense, dims (Nx, Ny, Nz); grid point (i, j, k) sits at origin + voxel * (i, j, k) (one multiply, one add, fp32) and has
 * the 64-bit linear index (i * Ny + j) * Nz + k -- the C order of a [Nx, Ny, Nz] tensor, z fastest.
 */
#ifndef DGS_MESH_OPS_H
#define DGS_MESH_OPS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGS_MESH_OPS_ABI_VERSION 2

int dgs_mesh_ops_abi_version(void);
const char* dgs_mesh_ops_last_error(void);

/* Fuse V views into the volume: ONE launch, the loop over the views inside the kernel, (tsdf, weight, colour) of a voxel in registers
 * and one store per voxel at the end.
 *   depth [V,H,W]   view-space z per pixel, 0 = nothing there;   rgb [V,3,H,W];   H, W >= 2
 *   proj  [V,16]    each camera's full_proj_transform as stored (row-vector convention: hom = [p, 1] @ proj)
 *   tsdf, weight [Nx*Ny*Nz];   color [Nx*Ny*Nz, 3] (three fp32 per voxel, not packed)
 *   accumulate = 0: the state starts at weight = prior_weight, tsdf = (prior_weight > 0 ? 1 : 0), colour 0 and is overwritten;
 *   accumulate = 1: the three arrays are read first, so views may be fed in chunks (bit-identical to one call).
 * Per voxel p and view, in this order, every operation a separately rounded fp32 one (the library is compiled with
 * -ffp-contract=off; dgs_amd/mesh.py states the same arithmetic in PyTorch):
 *   1. hom_c = p.x * proj[0][c] + ((p.y * proj[1][c] + p.z * proj[2][c]) + proj[3][c]) for c in {0, 1, 3};  z = hom_3;
 *      ndc = hom.xy / z;  reject unless z > 0 and -1 < ndc.x, ndc.y < 1
 *   2. u = ((ndc.x + 1) * W - 1) / 2, v likewise;  u0 = clamp(floor(u), 0, W - 2), fraction clamp(u - u0, 0, 1);  four depth taps,
 *      d = (d00 * (1 - fu) + d01 * fu) * (1 - fv) + (d10 * (1 - fu) + d11 * fu) * fv
 *   3. reject unless every tap satisfies 0 < tap <= depth_trunc
 *   4. sdf = d - z;  reject unless sdf > -trunc;  s = clamp(sdf / trunc, -1, 1)
 *   5. tsdf <- (tsdf * w + s) / (w + 1);  if sdf < trunc: colour <- (colour * w + bilinear rgb) / (w + 1);  w <- w + 1
 * Departures from the reference's torch fuser: (1) weights start at 0, not at 1 with a prior tsdf of 1 (prior_weight = 1 gives the
 * reference's start); (2) the pixel convention is the rasterizer's (pixel i's centre at ndc (2 i + 1) / W - 1), not
 * grid_sample(align_corners=True); (3) step 3 -- no interpolation across a silhouette into depth 0; (4) the colour is only
 * sampled where |sdf| < trunc (a view that sees the voxel as free space leaves its colour as it is).
 * No tap address can leave the view's image for any camera: taps are only formed from u0 in [0, W - 2], v0 in [0, H - 2]. */
int dgs_tsdf_integrate(int Nx, int Ny, int Nz, float origin_x, float origin_y, float origin_z, float voxel, int V, int H, int W,
                       const float* depth, const float* rgb, const float* proj, float trunc, float depth_trunc, float prior_weight,
                       int accumulate, float* tsdf, float* weight, float* color, void* stream);

/* Marching tetrahedra, pass 1.  Cell (i, j, k) (i < Nx-1 ...) has corner c at (i + (c & 1), j + (c >> 1 & 1), k + (c >> 2 & 1)) and is
 * cut into the six Kuhn tetrahedra {0, 1<<a, 1<<a | 1<<b, 7} of the permutations (a, b, c) of (0, 1, 2) in lexicographic order.
 * A cell is ACTIVE iff all 8 corners have weight > 0 and the corner signs (tsdf < 0) differ.
 *   cell_tris   [Nx*Ny*Nz] int32: triangles of the cell that starts at this grid point (0: inactive, or no cell starts here)
 *   point_mask  [Nx*Ny*Nz] uint8: bit (d - 1) set iff the edge from this grid point g to g + ((d & 1), (d >> 1 & 1), (d >> 2 & 1)),
 *               d in 1..7, carries a mesh vertex: its ends differ in sign and at least one active cell contains it
 *   point_verts [Nx*Ny*Nz] int32: number of set bits
 * A mesh vertex has the key (linear index of g) * 7 + (d - 1); its id is the rank of its key, the caller's inclusive prefix sums of
 * the two count arrays turn the counts into offsets. */
int dgs_mt_classify(int Nx, int Ny, int Nz, const float* tsdf, const float* weight, int* cell_tris, int* point_verts,
                    unsigned char* point_mask, void* stream);

/* Marching tetrahedra, pass 2.  cells [n_cells] / points [n_points]: ascending linear indices (int64) of the grid points with
 * cell_tris > 0 / point_mask != 0; tri_incl, vert_incl [Nx*Ny*Nz] int64: INCLUSIVE prefix sums of cell_tris and point_verts.
 *   vertices [Nv,3], vertex_colors [Nv,3] (color may be NULL, then vertex_colors is not written): position pa + t * (pb - pa) with
 *     t = fa / (fa - fb), a the edge's lower end; colour with the same t.  Ascending by key.
 *   faces [Nf,3] int32, ascending by (cell, tetrahedron, triangle within the tetrahedron).  One or three negative corners: the apex
 *     joined to the other three corners in ascending order; two negative corners a < b, non-negative c < d: the quad (a,c), (a,d),
 *     (b,d), (b,c) split along its first and third vertex.  Then wound so that the normal points from negative to positive tsdf. */
int dgs_mt_emit(int Nx, int Ny, int Nz, float origin_x, float origin_y, float origin_z, float voxel, const float* tsdf,
                const float* color, long long n_cells, const long long* cells, const int* cell_tris, const long long* tri_incl,
                long long n_points, const long long* points, const unsigned char* point_mask, const long long* vert_incl,
                float* vertices, float* vertex_colors, int* faces, void* stream);

/* Nearest neighbour of every query point in a reference set (brute force, all pairs).  For every query q
 *   best[q] = min over r in [0, n_ref) of ((unsigned long long)bits(d2(q, r)) << 32 | r)
 * with d2 = (dx * dx + dy * dy) + dz * dz, dx = q.x - r.x and so on, every operation a separately rounded fp32 one (the library is
 * compiled with -ffp-contract=off; dgs_amd/mesh_metrics.py: nearest_torch states the same arithmetic in PyTorch).  d2 >= 0, so its
 * bit pattern orders like its value: the packed minimum is the smallest distance and, among equal distances, the lowest
 * reference index.  The high word is the fp32 d2, the low word the index; every packed value is below 2^63.
 *   query [n_query,3], ref [n_ref,3] fp32;   best [n_query] -- set to all-ones on `stream` by this call before the launch
 *   ref_chunk: the reference set is cut into slices of ref_chunk points (the last one ragged), one grid row per slice; the
 *     slices meet in `best` through one 64-bit atomic minimum per query and slice, so the result does not depend on ref_chunk
 *     (values above n_ref mean one slice; dgs_nn_layout gives the default).
 * Refused with a negative status before any launch: n_ref < 1, n_ref >= 2^31, n_query < 0, ref_chunk < 1, a null pointer with a
 * non-zero count, more than 65535 slices.  n_query == 0 returns 0 and launches nothing.  Coordinates are expected to be finite (the
 * Python wrapper refuses others): a slice whose every d2 is NaN or +inf reports (+inf, first index of the slice).  A point of the
 * last, ragged round or slice is never read past n_ref: tails are index guards, no padded point exists that could win. */
int dgs_nn_search(long long n_query, const float* query, long long n_ref, const float* ref, long long ref_chunk,
                  unsigned long long* best, void* stream);

/* out = {queries per workgroup, reference points per LDS round, default ref_chunk}: the sizes at which the kernel changes path. */
int dgs_nn_layout(int out[3]);

/* Closest triangle of every query point (brute force, all pairs): the exact point-to-triangle distance behind
 * mesh_distance(mode="surface").  Version 2 libraries from this commit on also carry the dgs_tri_* pair; the version number is
 * unchanged because nothing that existed before changes.  For every query P
 *   best[P] = min over f in [0, n_tri) of ((unsigned long long)bits(d2(P, f)) << 32 | f)
 * -- the packing and the meaning of dgs_nn_search: the smallest squared distance and, among equal ones, the lowest face index.
 *
 * THE TABLE.  One row of fp32 values per triangle, computed once outside the kernel (dgs_amd/mesh_metrics.py: triangle_table,
 * elementwise PyTorch).  With corners A, B, C, dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z and
 * cross(a, b) = (a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x), every operation rounded on its own:
 *   e0 = B - A, e1 = C - B, e2 = A - C (edge k starts at O0 = A, O1 = B, O2 = C);   n = cross(e0, C - A);   m_k = cross(n, e_k)
 *   r_k = 1 / dot(e_k, e_k) where dot(e_k, e_k) > 0 and the quotient is finite, else 0;   rn = 1 / dot(n, n) under the same rule
 *   row = A, B, C, e0, e1, e2, n, m0, m1, m2 (three floats each), r0, r1, r2, rn, then two floats of padding (never read into the
 *   arithmetic): 34 values in a row of 36 floats = 144 bytes, a multiple of 16.  dgs_tri_layout reports the row length.
 *
 * THE PAIR.  For a query P and a row, every operation a separately rounded fp32 one (-ffp-contract=off; dgs_amd/mesh_metrics.py:
 * closest_face_torch states the same arithmetic in PyTorch):
 *   for k in 0..2:  w_k = P - O_k;  t = min(max(dot(w_k, e_k) * r_k, 0), 1);  c = w_k - t * e_k;  s_k = dot(c, c)
 *   best   = min(min(s_0, s_1), s_2)                                       the three edge segments
 *   inside = dot(w_0, m_0) >= 0 && dot(w_1, m_1) >= 0 && dot(w_2, m_2) >= 0 && rn > 0
 *   h = dot(w_0, n);  pl = (h * h) * rn                                     the plane, where P projects into the triangle
 *   d2 = inside ? min(pl, best) : best
 * No division and no branch per pair.  A triangle with collinear or coincident corners has rn = 0 and acts as its segments, a
 * zero-length edge has r_k = 0 and acts as its origin: no NaN.  d2 >= 0, so its bit pattern orders like its value.  Coordinates
 * are expected to be finite and of a size whose squares and fourth powers stay finite in fp32 (the Python wrapper refuses
 * non-finite ones); a pair whose d2 is NaN never wins.
 *   query [n_query,3] fp32;   table [n_tri,36] fp32, 16-byte aligned;   best [n_query] -- set to all-ones on `stream` by this call
 *   tri_chunk: slices of tri_chunk triangles (the last one ragged), one grid row per slice, merged in `best` by one 64-bit atomic
 *     minimum per query and slice, so the result does not depend on tri_chunk (values above n_tri mean one slice).
 * Refused with a negative status before any launch: n_tri < 1, n_tri >= 2^31, n_query < 0, tri_chunk < 1, a null pointer with a
 * non-zero count, a table that is not 16-byte aligned, more than 65535 slices.  n_query == 0 returns 0 and launches nothing.  A
 * triangle of the last, ragged round or slice is never read past n_tri: tails are index guards, no padded triangle exists that
 * could win. */
int dgs_tri_search(long long n_query, const float* query, long long n_tri, const float* table, long long tri_chunk,
                   unsigned long long* best, void* stream);

/* out = {queries per workgroup, triangles per LDS round, default tri_chunk, floats per table row}. */
int dgs_tri_layout(int out[4]);

/* Generalised winding number of a triangle mesh at every query point (brute force, all pairs): 1 inside a closed, outward-wound
 * mesh, 0 outside, -1 inside an inward-wound one, and a smooth value in between near an open rim -- the inside / outside test
 * behind contains, signed_distance and volume_iou of dgs_amd/mesh_metrics.py.  Version 2 libraries from this commit on also carry
 * the dgs_winding_* pair; the version number is unchanged because nothing that existed before changes (the precedent of dgs_tri_*).
 * For every query q
 *   sums[q] = sum over f in [0, n_tri) of (long long) rint(theta(q, f) * 2^28),      W(q) = sums[q] / (2 pi 2^28)
 * with theta half the signed solid angle of face f seen from q (van Oosterom and Strackee).  W is formed by the caller in float64, as one multiplication by 1 / (2 pi 2^28).
 *
 * THE TABLE.  One row of 12 fp32 values per triangle = 48 bytes, computed once outside the kernel (dgs_amd/mesh_metrics.py:
 * winding_table, elementwise PyTorch):  A, B, C, n = cross(B - A, C - A)  (three floats each; dot and cross as for dgs_tri_search,
 * every operation rounded on its own).  dgs_winding_layout reports the row length.
 *
 * THE PAIR.  Every operation a separately rounded fp32 one (-ffp-contract=off; dgs_amd/mesh_metrics.py: winding_sums_torch states
 * the same arithmetic in PyTorch), square roots and the division the correctly rounded IEEE ones:
 *   a = A - q, b = B - q, c = C - q;   la = sqrt(dot(a, a)), lb, lc likewise
 *   num = dot(a, n)             -- equal to the triple product a . (b x c) (b - a and c - a are the edges, whatever q is) without
 *                                  its cancellation: for a small, far triangle the triple product of three nearly parallel
 *                                  vectors loses about three digits
 *   den = ((la * lb) * lc + dot(a, b) * lc) + (dot(b, c) * la + dot(c, a) * lb)
 *   theta = ATAN2(num, den)
 * ATAN2(y, x) is written out, not left to a library:
 *   ay = |y|, ax = |x|;   r = min(ay, ax) / max(ay, ax), 0 where the maximum is 0;   s = r * r
 *   p = (((((((c7 s + c6) s + c5) s + c4) s + c3) s + c2) s + c1) s + c0) * r          (Horner, one rounding per operation)
 *     c0 = 1                         c1 = -0.3333165943622589       c2 = 0.19962704181671143      c3 = -0.13976581394672394
 *     c4 = 0.09794232249259949       c5 = -0.05777356028556824      c6 = 0.02304011397063732      c7 = -0.004355399403721094
 *   (the fp32 values nearest to these decimals; a minimax fit of atan on [0, 1] with c0 PINNED to 1: most pairs subtend tiny angles,
 *   where p = c0 r to rounding, so any other c0 is a relative bias of the whole sum -- an unconstrained fit puts every closed mesh at
 *   W = c0.  The fit's error is 5e-8 rad, 1.3e-7 rad with the roundings of the fp32 evaluation.)
 *   if ay > ax: p = PI_2 - p;   if x < 0: p = PI - p;   if y < 0: p = -p       (PI_2, PI: the fp32 values nearest to pi / 2 and pi)
 *   ATAN2 = p if y and x are both finite and not both zero, else 0 (a zero of either sign counts as not negative)
 * so a query on a vertex (num = den = 0), a NaN or infinite query and a NaN or infinite vertex add 0: every sum is finite.
 * THE SUM is an integer: theta * 2^28 is exact, rint rounds to nearest even, |term| < 2^30 and n_tri < 2^31 keep |sum| < 2^61.
 * Integer addition has no order, so the result is bit-identical from run to run, under any permutation or slicing of the faces,
 * and between the kernel and the PyTorch statement.
 *   query [n_query,3] fp32;   table [n_tri,12] fp32, 16-byte aligned;   sums [n_query] int64 -- set to zero on `stream` by this call
 *   tri_chunk: slices of tri_chunk triangles (the last one ragged), one grid row per slice, merged in `sums` by one 64-bit atomic
 *     add per query and slice (two's complement carries the sign), so the result does not depend on tri_chunk (values above
 *     n_tri mean one slice; dgs_winding_layout gives the default).
 * Refused with a negative status before any launch: n_tri < 1, n_tri >= 2^31, n_query < 0, tri_chunk < 1, a null pointer with a
 * non-zero count, a table that is not 16-byte aligned, more than 65535 slices.  n_query == 0 returns 0 and launches nothing.  A
 * triangle of the last, ragged round or slice is never read past n_tri.  No kernel waits for another, no trip count is read from
 * device memory.  Not a fast method: no tree, no multipole expansion, n_query * n_tri pairs. */
int dgs_winding_sum(long long n_query, const float* query, long long n_tri, const float* table, long long tri_chunk,
                    long long* sums, void* stream);

/* out = {queries per workgroup, triangles per LDS round, default tri_chunk, floats per table row}. */
int dgs_winding_layout(int out[4]);

/* Earth mover's distance between two point sets of the same size n: a minimum-cost perfect matching by a synchronous forward
 * auction with eps-scaling on INTEGER costs (dgs_amd/mesh_metrics.py: emd_torch states the same schedule in
 * PyTorch and the two agree bit for bit: assignment, prices, rounds).  Version 2 libraries from this commit on also carry the
 * dgs_emd_* pair; the version number is unchanged because nothing that existed before changes (the precedent of dgs_tri_*).
 *
 * COST.  c_ij = min(rint(sqrt((dx * dx + dy * dy) + dz * dz) * inv_q), 2^20) with dx = a_i.x - b_j.x and so on, every operation a
 * separately rounded fp32 one, the sqrt correctly rounded, rint to nearest even; then an integer in [0, 2^20].  inv_q = 1 / q,
 * q = diag / 2^20, diag the fp32 bounding-box diagonal of both sets together -- computed by the caller (mesh_metrics._emd_quantum);
 * inv_q = 0 (diag == 0) makes every cost 0.  Costs are recomputed on the fly: no n x n matrix exists.
 * SCHEDULE.  Prices p_j start at 0 and are kept across phases.  eps_0 = max(1, max_ij c_ij / 2) (integer division), then
 * eps <- max(1, eps / 4) until a phase with eps = 1 has run.  A phase starts with nobody assigned.  One ROUND: every unassigned i
 * bids at once against the prices at the start of the round: w_j = c_ij + p_j, j1 the lowest index that attains w1 = min_j w_j,
 * w2 = min over j != j1, bid = p_j1 + (w2 - w1) + eps.  Every object that received bids takes the largest packed word
 * bid << 24 | bidder (a 64-bit atomic maximum: the highest bid and, among equal bids, the highest bidder), its price becomes that
 * bid and its former owner becomes unassigned.  A phase ends when nobody is unassigned.  The rounds are synchronous and ties are
 * resolved by the packed words, so the result does not depend on scheduling.  Widths: bidder 24 bits (n < 2^24), bid 39 bits (the word stays below 2^63, like the packed minima above);
 * prices, bids and w are 64-bit integers throughout; a bid that would not fit 39 bits is detected (status -4), never wrapped.
 * At the end eps-complementary slackness holds with eps = 1, hence
 *   primal = sum_i c_{i,assignment(i)} <= OPT + n   and   dual = sum_i min_j (c_ij + p_j) - sum_j p_j <= OPT.
 *
 *   a, b [n,3] fp32 (persons, objects);   assignment [n] int32: the object of person i;   prices [n] int64 (both device memory)
 *   scratch: device memory, 8-byte aligned, at least dgs_emd_layout()[4] + n * dgs_emd_layout()[5] bytes; nothing is allocated here
 *   result [8] int64 in HOST memory: primal, dual, rounds, max cost, phases, last eps, and on status -3 the phase [4], its eps [5]
 *     and the persons still unassigned [6]
 * The host drives the rounds: two launches per round (bid, resolve), enqueued in batches; the unassigned count is read once per
 * batch (this call synchronises `stream`).  No kernel waits for another workgroup.  Rounds enqueued after a phase has converged
 * change nothing, and `rounds` counts only rounds that had bidders -- the count of the statement.
 * max_rounds caps the rounds over all phases: when a round would exceed it the call returns -3 with the phase, eps and bidders left
 * in the message; a partial matching is never returned as a result (assignment is then unspecified), and the same buffers may be
 * used for another call.  n == 0 and n == 1 launch nothing (n == 1: the trivial matching, the cost computed on the host).
 * Refused with a negative status before any launch: a null pointer with n > 0 (scratch with n > 1), n < 0, n >= 2^24,
 * max_rounds <= 0, inv_q negative or not finite, a scratch buffer too small or misaligned.  No address can leave an array: every
 * index is a person or an object below n (list entries are written from [0, n) only, a list holds at most n of them). */
int dgs_emd_auction(long long n, const float* a, const float* b, float inv_q, long long max_rounds, void* scratch,
                    long long scratch_bytes, int* assignment, long long* prices, long long* result, void* stream);

/* out = {threads per workgroup, objects per LDS round of the dense bidding kernel, the bidder count up to which the sparse bidding
 *        kernel (a workgroup per bidder) runs, entries of `result`, fixed bytes of scratch, bytes of scratch per point}. */
int dgs_emd_layout(int out[6]);

/* Z-buffer rasterizer of a triangle mesh: which face is nearest at every pixel centre, its depth, its barycentrics and the
 * perspective-correct interpolation of per-vertex attributes -- the images of dgs_amd/mesh_render.py (the role nvdiffrast has in
 * the reference's render_mesh.py:221-240).  Not differentiable.  Version 2 libraries from this commit on also carry the
 * dgs_mesh_raster* / dgs_mesh_resolve calls; the version number is unchanged because nothing that existed before changes (the
 * precedent of dgs_tri_*).  Every operation below is a separately rounded fp32 one (-ffp-contract=off), divisions, ceil and floor
 * the IEEE ones; dgs_amd/mesh_render.py: raster_table / rasterize_torch / interpolate state the same arithmetic in PyTorch.
 *
 * VERTEX.  With m the camera's full_proj_transform as stored and p the vertex:
 *   hom_c = p.x * m[0][c] + ((p.y * m[1][c] + p.z * m[2][c]) + m[3][c]) for c in {0, 1, 3}   (the expression of dgs_tsdf_integrate)
 *   w = hom_3 (the view depth);   sx = ((hom_0 / w + 1) * W - 1) / 2,  sy likewise with H;   iw = 1 / w
 * -- the rasterizer's pixel convention: the centre of pixel (i, j) is the screen point (i, j).
 *
 * FACE (v0, v1, v2).  Dropped if any corner has w <= near or a non-finite screen coordinate.  No clipping (a stated departure: the
 * meshes of the protocol lie in front of the camera).  Edge k is the edge opposite corner k; its two endpoints are put in the
 * canonical order a < b, lexicographic by screen coordinates (x, then y) -- vertex ids are not used -- and
 *   e_k(P) = s_k * ((xb - xa) * (P.y - ya) - (yb - ya) * (P.x - xa)),   s_k = -1 if that order reversed the face's own order
 *   (v_{k+1} to v_{k+2}), else +1.
 * Two faces that share an edge compute the same number with opposite signs, welded or not: a pixel centre off the edge belongs to
 * exactly one of them, one exactly on it to both; no crack between neighbours.  A = e_0(v0); a face with A == 0 (or NaN) is dropped.
 * Pixel P = (i, j) is COVERED when it lies in the face's pixel box [ceil(min x), floor(max x)] x [ceil(min y), floor(max y)]
 * intersected with the image, the three e_k are all >= 0 (A > 0) or all <= 0 (A < 0), S = (e_0 + e_1) + e_2 != 0 and, with
 *   b_k = e_k / S;   q = (b_0 * iw_0 + b_1 * iw_1) + b_2 * iw_2;   z = 1 / q       (the perspective-correct view depth)
 * q > 0: so z > 0, and a pixel whose q is NaN -- an edge function that overflowed to an infinity gives b = inf / inf -- is not covered.
 * PIXEL.  best[P] = min over the covering faces of ((unsigned long long)bits(z) << 32 | face): the nearest face and, among equal
 * depths, the lowest face index; all-ones where nothing covers P.  No back-face culling.
 * ATTRIBUTES of the winning face (C channels per vertex, b and z recomputed by the same expressions):
 *   a = (((b_0 * iw_0) * a_0 + (b_1 * iw_1) * a_1) + (b_2 * iw_2) * a_2) * z
 *
 * THE TABLE.  One row of 24 four-byte values per face = 96 bytes, a multiple of 16, computed once outside the kernels by
 * elementwise PyTorch (raster_table); dgs_mesh_raster_layout reports the row length:
 *    0.. 3   xa, ya, xb - xa, yb - ya of edge 0          4.. 7   of edge 1          8..11   of edge 2
 *   12..15   s_0, s_1, s_2, sign of A (+1 / -1; 0 for a dropped face)
 *   16..19   iw_0, iw_1, iw_2, one float of padding (never read into the arithmetic)
 *   20..23   the pixel box x0, x1, y0, y1 as int32, already intersected with the image; (0, -1, 0, -1) for a dropped face or an
 *            empty box
 *
 * dgs_mesh_raster: coverage of the faces named by `list` into best [H*W].  Two paths: path 0, one lane per face and a loop over its
 * box, for faces of small boxes; path 1, one or more workgroups per face whose threads stride over the box, for large ones.  Both
 * compute the same numbers and meet in `best` through the 64-bit atomic minimum (behind a plain load: the atomic is only issued
 * when the candidate is smaller), so any face may go through either path and the result does not depend on the split; the caller
 * puts the faces whose box holds at most dgs_mesh_raster_layout()[0] pixels on path 0 and leaves faces with an empty box out.
 *   table [n_faces,24] 16-byte aligned;   list [n_list] int32 face indices (entries outside [0, n_faces) are skipped)
 *   clear != 0: best is set to all-ones on `stream` first, so a second call with clear = 0 adds the other path's faces to the
 *   same buffer.  n_list == 0 is legal: only the clear happens.
 * No address can leave `best`: the kernels clamp every box to the image again before they form a pixel index.
 * Refused with a negative status before any launch: H or W < 1, H * W > 2^30, n_faces < 0 or >= 2^31 (the face is the low 32 bits
 * of the packed minimum), n_list < 0 or >= 2^31, a path other than 0 or 1, a null pointer with a non-zero count, a table that is
 * not 16-byte aligned. */
int dgs_mesh_raster(long long n_faces, const float* table, const int* list, long long n_list, int path, int H, int W,
                    unsigned long long* best, int clear, void* stream);

/* One thread per pixel: unpack best [H*W], recompute the winner's b and z and interpolate.  Outputs (any may be NULL and is then
 * not written):
 *   face_id [H*W] int32, -1 where nothing was drawn;   depth [H*W], 0 there;   bary [H*W,3], 0 there
 *   image [C,H*W]: the interpolated attributes, background[c] where nothing was drawn
 *   faces [n_faces,3] int32 vertex ids;  attr [n_vertices,C];  background [C] (device memory).  C in [0, 8]; with C == 0 the four
 *   attribute arguments are not read.  A pixel whose packed face is not below n_faces counts as empty; a face that names a vertex
 *   outside [0, n_vertices) gets the background.
 * Refused with a negative status before any launch: H or W < 1, H * W > 2^30, n_faces or n_vertices < 0 or >= 2^31, C outside
 * [0, 8], a null pointer with a non-zero count, a table that is not 16-byte aligned. */
int dgs_mesh_resolve(int H, int W, const unsigned long long* best, long long n_faces, const float* table, const int* faces,
                     long long n_vertices, const float* attr, int C, const float* background, int* face_id, float* depth, float* bary,
                     float* image, void* stream);

/* out = {largest box area (pixels) of path 0, threads per workgroup (both paths and the resolve), floats per table row,
 *        largest C}: the sizes at which the code changes path. */
int dgs_mesh_raster_layout(int out[4]);

/* Connected components of a graph given as groups of nodes: the primitive behind dgs_amd/mesh_clean.py (the component filter on the
 * device, cluster_connected_triangles, clean_mesh -- the role open3d's cluster_connected_triangles has in the reference's
 * utils/mesh_utils.py:24-45 and render_mesh_trajectory.py:41-88).  Version 2 libraries from this commit on also carry the dgs_cc_*
 * pair; the version number is unchanged because nothing that existed before changes (the precedent of dgs_tri_* and
 * dgs_mesh_raster*).
 *   groups [n_groups,k] int32, k in {2, 3}: all nodes named by one group are in the same component.  The faces [F,3] of a mesh are
 *     the k = 3 input as they stand (components over shared vertices); no edge list is materialised.  Repeated groups and groups
 *     that name a node twice are legal.  An id outside [0, n_nodes) is skipped by an index guard (the rest of its group still
 *     counts), so no address can leave `label`; the Python wrapper refuses such input.
 *   label [n_nodes] int32: on return label[i] is the SMALLEST NODE ID of i's component; a node that no group names keeps its own id.
 * The answer is unique, so it cannot depend on the order in which the atomics land: it is bit-identical from run to run and equal
 * to the NumPy / PyTorch statement (dgs_amd/mesh_clean.py: component_labels on CPU tensors, dgs_amd/mesh.py: vertex_components).
 *
 * Three launches on `stream`, no host read between them:
 *   init      label[i] = i
 *   hook      lock-free union-find, a thread per group: for each of the k - 1 pairs (first node, other node) find both roots; while
 *             they differ, atomicCAS(&label[hi], hi, lo) with hi the larger root.  A failed CAS writes nothing and returns hi's true
 *             parent; the walk continues from there.
 *   compress  label[i] = root(i), in place.
 * INVARIANT: label[x] <= x at all times, and label[x] is a node of x's component.  Only a successful CAS lowers an entry during the
 * hook, and only on a node that is a root at that instant (the compare value is the node's own id); the compress only replaces an
 * entry by the same node's root.  Every walk x -> label[x] -> ... therefore strictly descends and ends at a node r with
 * label[r] == r: every loop is finite.  When the hook has finished, each component is one tree (every pair of every group went
 * through a successful CAS or was found under a common ancestor) and its root is its smallest node: the smallest node m has
 * label[m] <= m inside its own component, hence label[m] == m.
 * Memory scope.  The XCD L2s are not coherent with each other and a CU's L1 is never refreshed by another CU, so the walks use
 * relaxed agent-scope atomic loads (32-bit, no inline assembly).  Correctness does not rest on their freshness: any value a load
 * can return was the entry at some instant since the init launch, so it is an ancestor in the same component; a walk over stale
 * values ends at an ancestor that merely looked like a root, and the CAS -- executed at the memory side on the true value --
 * decides: it fails and hands back the true parent, and after each failed CAS the larger of the two candidates is strictly smaller
 * than before.  The CAS result, not a load, ends the loop, so a load that stays stale for the whole launch cannot keep a thread
 * spinning.
 * The compress runs in place: no hook runs beside it, so the roots are fixed; a thread that meets a chain another thread has half
 * compressed reads, per entry, either the old parent or the root, both ancestors on the way to the same root, and still ends there.
 * Refused with a negative status before any launch: k outside {2, 3}, a negative count, n_nodes >= 2^31, a null pointer with a
 * non-zero count.  n_nodes == 0 returns 0 and launches nothing; n_groups == 0 runs only the init. */
int dgs_cc_labels(long long n_nodes, const int* groups, long long n_groups, int k, int* label, void* stream);

/* out = {threads per workgroup, groups per thread}: a workgroup takes out[0] * out[1] groups -- the sizes at which the code changes
 * path (a second workgroup, a ragged last one). */
int dgs_cc_layout(int out[2]);

/* Mesh simplification by vertex clustering with quadric placement: the kernels behind dgs_amd/mesh_simplify.py (open3d's
 * simplify_vertex_clustering(contraction=Quadric / Average), which the reference's users reach for before printing a mesh).
 * Version 2 libraries from this commit on also carry the dgs_simplify_* triple; the version number is unchanged because nothing
 * that existed before changes.  THE STATEMENT -- every fp operation rounded on its own, fp32 unless it says fp64; rn() is
 * round-to-nearest-even to an integer; dgs_amd/mesh_simplify.py states the same arithmetic in PyTorch and CPU tensors run it:
 *
 * 1. CELLS (the wrapper: PyTorch on the tensors' device).  origin defaults to the per-axis minimum of the vertices - cell / 2;
 *    ijk = floor((v - origin) / cell), each component in [0, 2^21); the cluster id of a vertex is the rank of its (i, j, k) among
 *    the occupied cells in ascending lexicographic order; centre = origin + (ijk + 0.5) * cell.
 * 2. SUMS (dgs_simplify_accumulate).  rows [n_clusters,16] int64, one row per cluster:
 *      column 0        the number of vertices of the cluster
 *      columns 1..3    sum over its vertices of rn(((v - centre) / cell) * 2^30), per axis
 *      columns 4..6    sum over its vertices of rn(clamp(colour, 0, 1) * 2^24), a NaN colour counting as 0 (0 without colours)
 *      columns 7..12   A: xx xy xz yy yz zz;   columns 13..15   b
 *    Per face (a, b, c): n = (b - a) x (c - a), each component a difference of two rounded products (n.x = e1.y e2.z - e1.z e2.y
 *    ...); l = fp32(sqrt(fp64((n.x n.x + n.y n.y) + n.z n.z))) -- the fp64 square root, because it is correctly rounded on the
 *    device and on the host while the device's fp32 one is not.  A face counts iff 0 < l < inf.  nh = n / l per component;
 *    w = min((0.5 l) / (cell cell), W_MAX).  For every distinct cluster k among the three corners, with m the number of corners in
 *    k and p the first of them: u = (p - centre_k) / cell;  d = -((nh.x u.x + nh.y u.y) + nh.z u.z);  the row of k receives
 *    m * rn(((w nh_i) nh_j) * 2^Q) for i <= j and m * rn(((w d) nh_i) * 2^Q).  All sums are integer additions: their order and
 *    grouping cannot change a bit, which is what lets the kernel combine neighbouring lanes on chip and still be equal to the
 *    PyTorch statement.
 *    Q = 24, W_MAX = 16 (a face of 16 cell areas; larger faces are weighted as that).  NO SUM CAN OVERFLOW for any mesh the library
 *    accepts (fewer than 2^31 vertices and fewer than 2^31 faces, hence fewer than 3 * 2^31 corner incidences in one cell):
 *      - count < 2^31.
 *      - |u| < 2 per axis: the vertex lies in its cell up to the rounding of steps 1 (ijk < 2^21 and 24-bit significands put
 *        (v - origin) / cell and the centre each within 2^21 * 2^-23 = 1/4 cell of their exact values), so |u| <= 1/2 + 1/4 + 1/4
 *        and a rounding; a position term is below 2^31, a sum below 2^62.
 *      - a colour term is at most 2^24, a sum below 2^55.
 *      - |nh_i| <= 1 + 2^-22, so |w nh_i nh_j| < 1.001 W_MAX and a term of A is below 1.001 * 2^28 + 1/2; |d| <= |nh| |u| <
 *        1.001 * 2 sqrt(3) < 3.5, so a term of b is below 3.5 * 2^28 + 1/2; 3 * 2^31 of them stay below 10.5 * 2^59 + 2^32 < 2^63.
 * 3. SOLVE (dgs_simplify_solve), per cluster in fp64.  An int64 is converted to fp64 by one rounding.  The sums enter as they are:
 *    the solution does not change when A and b are scaled together, so 2^-Q is never applied.
 *      xb_i = clamp(pos_i / (count * 2^30), -1, 1)                          (0 where count = 0)
 *      placement 0 (average): x = xb.   placement 1 (quadric):
 *      t = (a00 + a11) + a22;  g = t * 2^-10;  m00 = a00 + g, m11 = a11 + g, m22 = a22 + g;  r_i = g * xb_i - b_i
 *      c00 = m11 m22 - a12 a12   c01 = a02 a12 - a01 m22   c02 = a01 a12 - a02 m11
 *      c11 = m00 m22 - a02 a02   c12 = a01 a02 - m00 a12   c22 = m00 m11 - a01 a01
 *      det = (m00 c00 + a01 c01) + a02 c02
 *      x0 = ((c00 r0 + c01 r1) + c02 r2) / det,  x1 = ((c01 r0 + c11 r1) + c12 r2) / det,  x2 = ((c02 r0 + c12 r1) + c22 r2) / det
 *      x = xb unless t > 0, 0 < det < inf and every |x_i| <= 1 (a NaN fails).
 *    That is (A + lambda t I) x = -b + lambda t xb with lambda = 2^-10: the minimiser of the summed squared plane distances, pulled
 *    to the cluster mean along the directions the planes leave free (flat and creased regions, where A has rank 1 or 2).
 *    vertex = centre + fp32(x) * cell (fp32);  colour = fp32(col_i / (count * 2^24)).  Every output vertex lies within one cell of
 *    its cell centre per axis.
 * 4. FACES (the wrapper: PyTorch): every index replaced by its cluster; faces that name a cluster twice and later repeats of a face
 *    up to rotation dropped; unreferenced vertices dropped; order and winding kept.
 *
 * dgs_simplify_accumulate: vertices [n_vertices,3], colors [n_vertices,3] or null, faces [n_faces,3] int32, cluster [n_vertices]
 * int32, centres [n_clusters,3], rows [n_clusters,16] int64 (cleared by the call).  Up to three operations on `stream`: the clear,
 * a launch over the vertices, a launch over the faces.  A workgroup keeps its items' keys and values in LDS, finds the runs of
 * neighbouring items with one cluster, and sums every run on chip; a run then costs one 64-bit atomic per non-zero column, 16 lanes
 * on the 128 contiguous bytes of one row (csrc/mesh_common.h).  A vertex id outside [0, n_vertices) drops its face, a cluster
 * id outside [0, n_clusters) drops that vertex or that corner's contribution: index guards, so no address leaves a buffer; the
 * Python wrapper produces no such ids.
 * Refused with a negative status before any launch: a negative count, a count >= 2^31, cell not positive and finite, a null pointer
 * with a non-zero count, a placement outside {0, 1}.  n_clusters == 0 returns 0 and launches nothing; a zero n_vertices or n_faces
 * skips that launch. */
int dgs_simplify_accumulate(long long n_vertices, const float* vertices, const float* colors, long long n_faces, const int* faces,
                            const int* cluster, long long n_clusters, const float* centres, float cell, long long* rows, void* stream);

/* rows, centres as above -> vertices [n_clusters,3] and, unless null, colors [n_clusters,3].  One launch, a thread per cluster. */
int dgs_simplify_solve(long long n_clusters, const long long* rows, const float* centres, float cell, int placement, float* vertices,
                       float* colors, void* stream);

/* out = {threads per workgroup, items per thread, Q, W_MAX, the exponent of lambda (-10)}: a workgroup takes out[0] * out[1] vertices
 * or faces. */
int dgs_simplify_layout(int out[5]);

/* Mesh smoothing: the Jacobi steps behind dgs_amd/mesh_smooth.py (the roles of open3d's filter_smooth_simple, filter_smooth_laplacian
 * and filter_smooth_taubin, which the reference's users reach for to take the voxel staircase off an extracted surface).  Version 2
 * libraries from this commit on also carry the dgs_smooth_* pair; the version number is unchanged because nothing that existed
 * before changes (the precedent of dgs_tri_*).  UNIFORM (umbrella) WEIGHTS ONLY -- a stated departure from any distance- or
 * cotangent-weighted variant: every neighbour counts the same, whatever the edge lengths.
 *
 * THE ADJACENCY (the wrapper: PyTorch on the tensors' device, dgs_amd/mesh_smooth.py: vertex_adjacency).  A CSR table: offsets
 * [n_vertices + 1] int64, neighbours [n_entries] int32; row i = neighbours[offsets[i] .. offsets[i + 1]) lists the distinct vertices
 * j != i that share a face with i, ASCENDING.  Repeated faces do not repeat a neighbour; a face that names a vertex twice is legal.
 *
 * ONE STEP, for all C channels of x [n_vertices,C] fp32 and row i of length d, every operation a separately rounded fp32 one
 * (-ffp-contract=off), the division the IEEE one:
 *   acc = 0;  for k in row order: acc = acc + x[neighbours[k]]                (sequential per channel)
 *   mode 0 (laplacian), factor s:  out = x + s * (acc / float(d) - x)
 *   mode 1 (simple):               out = (x + acc) / float(d + 1)             (the factor is not used)
 *   out = x where d == 0 or pinned[i] != 0.
 * Every step reads the complete output of the step before it (Jacobi, never in place).  dgs_amd/mesh_smooth.py: smooth_steps_torch
 * states the same arithmetic in PyTorch, slot by slot of the rows, and CPU tensors run it: the results are bit-identical.  The order
 * of a row's sum follows the vertex ids, so THE LAST BITS OF THE RESULT DEPEND ON THE VERTEX NUMBERING: renumbering a mesh changes
 * them (and nothing else).  laplacian x n: n steps with lam;  taubin x n: n times (a step with lam, a step with mu), 2 n steps;
 * simple x n: n steps of mode 1.
 *
 * dgs_smooth_steps: one call enqueues all n_steps launches on `stream`, step k with factors[k], ping-ponging between x and tmp
 * [n_vertices,C] (two different buffers: no launch reads what it writes, no kernel waits for another workgroup).  THE RESULT IS
 * ALWAYS IN x: an odd count ends with one device-to-device copy on the same stream; tmp holds unspecified values afterwards.
 *   factors [n_steps]: HOST memory, read before the call returns;   pinned [n_vertices] bytes in device memory, or NULL for none
 *   C in [1, 8]: a thread per vertex keeps its C sums in registers.  A row of thousands of entries (the hub of a fan) is walked by
 *   one thread: correct, and as slow as that sounds.
 * A row range is clamped to [0, n_entries] and a neighbour id outside [0, n_vertices) adds nothing: index guards, so no address can
 * leave a buffer; the Python wrapper produces no such input.
 * Refused with a negative status before any launch: a negative count, n_vertices or n_entries >= 2^31, C outside [1, 8], a mode
 * other than 0 or 1, n_steps above dgs_smooth_layout()[3], a null pointer with a non-zero count, a factor that is not finite.
 * n_steps == 0 or n_vertices == 0 returns 0 and launches nothing. */
int dgs_smooth_steps(long long n_vertices, const long long* offsets, const int* neighbours, long long n_entries, int C, int mode,
                     const float* factors, int n_steps, const unsigned char* pinned, float* x, float* tmp, void* stream);

/* out = {threads per workgroup, vertices per workgroup, largest C, largest n_steps of one call}. */
int dgs_smooth_layout(int out[4]);

/* Mesh decimation: quadric edge collapse in synchronous rounds, the kernels behind dgs_amd/mesh_decimate.py (the role of open3d's
 * simplify_quadric_decimation(target_number_of_triangles): "this surface at N faces, still a manifold").  Version 2 libraries from
 * this commit on also carry the dgs_decimate_* calls; the version number is unchanged because nothing that existed before changes
 * (the precedent of dgs_tri_*).  THE STATEMENT -- every fp operation rounded on its own (-ffp-contract=off), fp32 or fp64 as it
 * says; rn() is round-to-nearest-even to an integer; an int64 is converted to fp64 by one rounding; dgs_amd/mesh_decimate.py states
 * the same arithmetic in PyTorch and CPU tensors run it.  Every step is defined so that the order in which threads run cannot
 * change a bit: sums are integer sums, ties are decided by minima of distinct 64-bit keys, and a round only reads what the round
 * before it finished.
 *
 * 0. FRAME AND LOCKS (the wrapper).  Faces that name a vertex twice are dropped.  centre = (min + max) * 0.5 per axis (fp32);
 *    scale = 2^-e with e the binary exponent of the largest half extent h (h = m 2^e, 1/2 <= m < 1; e clamped to [-100, 100];
 *    scale = 1 if h = 0); pos = (v - centre) * scale, so |pos_i| <= 1 + 2^-22: one rounding in the subtraction, none in the
 *    product.  A vertex that no collapse has moved is returned with its input bits; a moved one as centre + pos * (1 / scale).
 *    Per round, from the edges of the current faces: a vertex is on the BOUNDARY if it lies on an edge used by one face, and
 *    LOCKED if it lies on an edge used by more than two faces, or on the boundary while preserve_boundary is set.  A locked vertex
 *    never moves and never disappears.  flags [V] bytes: bit 0 locked, bit 1 boundary.
 * 1. INITIAL QUADRICS (dgs_decimate_quadrics).  rows [V,10] int64: A (xx xy xz yy yz zz), b (x y z), c.  Per face (a, b, c), in
 *    fp32 as in dgs_simplify_accumulate: n = (b - a) x (c - a), each component a difference of two rounded products;
 *    l = fp32(sqrt(fp64((n.x n.x + n.y n.y) + n.z n.z))); the face counts iff 0 < l < inf; nh = n / l; w = min(l / mean_len, W_MAX).
 *    mean_len is the caller's: fp32(fp64(sum over the countable faces of ceil(fp64(l) 2^28)) / count * 2^-28), an integer sum; the
 *    ceil makes it no smaller than the true mean, so the weights of a mesh sum to at most F (1 + 2^-22).  Then in fp64 (W, N, P the
 *    fp32 values w, nh, pos[a] converted): d = -((N.x P.x + N.y P.y) + N.z P.z) and the row of EACH of the three corners receives
 *    rn(((W N_i) N_j) 2^Q) for i <= j, rn(((W d) N_i) 2^Q) and rn(((W d) d) 2^Q).
 *    Q = q_bits = min(40, 59 - ceil(log2 F)) is chosen by the caller from the face count F of the input: a mesh of 10^6 faces has
 *    Q = 39 and resolves squared distances of 2^-39 of the frame.  W_MAX = 16.  A collapse ADDS the two vertices' rows (Garland and
 *    Heckbert's accumulated quadrics); rows are never recomputed from the current faces.
 *    NO SUM CAN OVERFLOW.  |N_i| <= 1 + 2^-22, |P_i| <= 1 + 2^-22, so |d| < 1.74 and a term is below W (3.02 * 2^Q) + 1/2 in
 *    magnitude (the largest is W d d).  Whatever is merged, a row is a sum of initial contributions, and every face contributes to
 *    three rows once: |row entry| <= 3 * (sum of W) * 3.02 * 2^Q + 3 F / 2 <= 9.07 F 2^Q + 1.5 F < 2^4 * 2^59 = 2^63, because the
 *    calls refuse q_bits unless F * 2^q_bits <= 2^59.  (W_MAX is not needed for this bound; it keeps one huge face from owning the
 *    regularisation of its neighbours.)
 * 2. A ROUND.
 *    a. EDGES (the wrapper: sorts, run lengths and prefix sums on the tensors' device; mesh_decimate.round_tables).  edges [5,E]
 *       int32, one COLUMN per distinct undirected edge of the current faces, ascending by (u, v): row 0 u, row 1 v (u < v), row 2
 *       the number of faces at the edge, rows 3 and 4 the vertex opposite the edge in the first and in the second of those faces,
 *       faces in ascending order (-1 where there is no second face).  The CSR vertex adjacency (adj_offsets [V+1] int64, adj [2E]
 *       int32, rows ascending) and the faces of every vertex (vf_offsets [V+1] int64, vf [3F] int32, rows ascending).
 *    b. COST AND PLACEMENT (dgs_decimate_edges, a thread per edge, fp64).  r = fp64(row_u + row_v) (an integer sum); pu, pv the
 *       endpoints, mid = (pu + pv) * 0.5.  The regularised system of dgs_simplify_solve with xb = mid:
 *         t = (a00 + a11) + a22;  g = t * 2^-10;  m00 = a00 + g, m11 = a11 + g, m22 = a22 + g;  r_i = g * mid_i - b_i
 *         c00 .. c22, det and y as there (x0 = ((c00 r0 + c01 r1) + c02 r2) / det ...)
 *         rad = (|pv.x - pu.x| + |pv.y - pu.y|) + |pv.z - pu.z|
 *         x = y if t > 0, 0 < det < inf and every |y_i - mid_i| <= rad (a NaN fails), else mid -- the edge's neighbourhood is the
 *         box of half width rad around its midpoint;  x = pu if u is locked, else pv if v is locked.
 *       Both locked: the edge is no candidate (cost 0, place 0, valid 0).  place = fp32(x), and with X = fp64(place):
 *         q_i = (a_i0 X0 + a_i1 X1) + a_i2 X2;  raw = (((X0 q0 + X1 q1) + X2 q2) + 2 * ((b0 X0 + b1 X1) + b2 X2)) + c
 *         cost = fp32((raw > 0 ? raw : 0) * 2^-Q)                    -- the weighted squared distance, in the frame's units
 *       An edge is no candidate if raw is NaN or cost > max_cost (the caller's fp32((max_error * scale)^2); +inf for no bound).
 *    c. VALIDITY (the same launch), for candidates:
 *       - count <= 2, the two opposite vertices differ, and an edge with two faces does not join two boundary vertices (collapsing
 *         such a chord would pinch the surface).
 *       - VALENCE.  Every opposite vertex has at least 5 neighbours, or at least 3 if it is on the boundary.  After the collapse it
 *         has one fewer: an interior vertex keeps at least four faces and a boundary one at least one.  The textbook condition
 *         asks for more than 3 -- otherwise two faces end up on one vertex set and a tetrahedron would lose its volume -- and would
 *         let an octahedron collapse to a double pyramid over a triangle, whose apexes sit on three faces each; asking for 5 keeps
 *         every vertex of a closed surface on four faces or more and returns the tetrahedron and the octahedron unchanged.
 *       - LINK.  The common neighbours of u and v (a merge of their two ascending rows) are exactly the opposite vertices: as many
 *         as the edge has faces, and none other.
 *       - FLIP.  For every face at u, then at v, that does not hold both (those go with the edge): with p the corners as they are
 *         and q the corners with u or v replaced by X, n0 = (p1 - p0) x (p2 - p0), n1 = (q1 - q0) x (q2 - q0) in fp64,
 *         (n0.x n1.x + n0.y n1.y) + n0.z n1.z > 0.  A face whose new area is zero fails, and so does one that had none.
 *    d. THROTTLE (the wrapper).  An edge competes iff it is valid and cost <= the k-th smallest valid cost,
 *       k = ceil(ceil((F - target) / 2) * oversubscribe), by torch.kthvalue: a locally cheapest but globally expensive edge waits.
 *    e. INDEPENDENT SET (dgs_decimate_select).  key = bits(cost) << 32 | scramble(edge id); cost >= 0, so its bit pattern orders
 *       like its value and key < 2^63.  scramble(i): h = i * 0x9E3779B1; h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13 (mod 2^32) -- a
 *       bijection, so keys are distinct.  A stated departure from "the edge id breaks ties": on a flat region every cost is 0, the
 *       edge order has a single local minimum there and a round would select one edge; a scrambled id gives a pseudo-random order
 *       with a local minimum every few dozen edges.  It still is a function of the edge id alone.
 *         pass 1:  m1[x] = min of the keys of the competing edges at x (NO_KEY = 2^63 - 1 where there is none): the 64-bit atomic
 *                  minimum behind a plain load.
 *         pass 2, over ALL edges (u, v), competing or not, m2 starting as a copy of m1:  m2[u] <- min(m2[u], m1[v]) and
 *                  m2[v] <- min(m2[v], m1[u]), so m2[x] = min(m1[x], m1[y] for y adjacent to x).
 *         pass 3:  an edge is SELECTED iff it competes and m2[u] == m2[v] == key.
 *       PROOF OF INDEPENDENCE.  (1) A selected edge e = (u, v) competes at u, so m1[u] <= key(e); m2[u] = key(e) <= m1[u] gives
 *       m1[u] = key(e), and likewise m1[v] = key(e).  (2) Two selected edges e != e' cannot share an endpoint x: m1[x] would equal
 *       two distinct keys.  (3) Nor can an endpoint x of e be adjacent to an endpoint x' of e': m2[x] <= m1[x'] = key(e') and
 *       m2[x'] <= m1[x] = key(e) give key(e) <= key(e') <= key(e).  So no face touches two selected edges (two of its corners would
 *       be equal or adjacent endpoints), no vertex adjacent to an endpoint of e moves or disappears in this round, and the rows,
 *       faces and positions that (c) read for e are the ones the collapse meets: the checks stay true when all selected collapses
 *       are applied at once.  (A vertex opposite two selected edges loses a neighbour to each; its ring then holds two disjoint,
 *       non-adjacent edges, hence six vertices or five on a boundary, and it keeps four, or three on the boundary.)
 *       If the selected collapses would remove more faces than F - target, the wrapper applies only the cheapest by key, for as long
 *       as the faces removed so far are fewer than F - target: the count ends at target or target - 1.
 *    f. APPLY (dgs_decimate_apply: a thread per selected edge, then a thread per face).  The survivor s is u, the smaller id --
 *       unless v alone is locked, then it is v, so that a locked vertex keeps its id, its position and its colour -- and the other
 *       endpoint d merges into it: pos[s] = place; row[s] = row[u] + row[v]; moved[s] = 1 unless an endpoint is locked;
 *       colour[s] = c_u + t * (c_v - c_u) in fp32 with t = fp32(clamp(((X - pu) . (pv - pu)) / ((pv - pu) . (pv - pu)), 0, 1)) in
 *       fp64 (a NaN counts as 0); vmap[d] = s (vmap is the identity elsewhere).  Then every face is re-indexed through vmap and
 *       keep[face] = its three ids differ.  The wrapper drops the others and keeps the order.
 *    g. STOP.  The face count has reached the budget, a round selects nothing, or max_rounds rounds have run.  The host reads the
 *       sizes of the round's lists (the selected edges, the kept faces) once per round.
 * 3. OUTPUT (the wrapper).  Surviving vertices in ascending input id, surviving faces in their order and winding.
 *
 * Arguments.  All device memory.  pos [V,3] fp32 (the frame), rows [V,10] int64, flags / moved / valid / compete / selected / keep
 * bytes, faces [F,3] int32, edges [5,E] int32, cost [E] fp32, place [E,3] fp32, m1 / m2 [V] 64-bit words, vmap [V] int32, sel
 * [n_sel] int32 edge ids, colors [V,3] fp32 or NULL.  dgs_decimate_quadrics clears rows first; dgs_decimate_select writes m1, m2 and
 * selected (five operations on `stream`); dgs_decimate_apply writes vmap and keep and updates pos, rows, colors, moved and faces in
 * place (three launches).  No kernel waits for another workgroup; every loop is over a row whose range is clamped to its array.
 * GUARDS.  Every id read from a buffer is range-checked before an address is formed from it: a face with a vertex id outside [0, V)
 * adds nothing to the rows and keeps that id when it is re-indexed; an edge with such an endpoint, or with u == v, gets cost 0,
 * place 0, valid 0, takes no part in the selection and is skipped by the apply; an opposite vertex, a face id or a face's vertex
 * outside its range makes the edge invalid; a selected entry outside [0, E) is skipped.  A row range is clamped to [0, n_adj] or
 * [0, n_vf].  The Python wrapper produces no such input.
 * Refused with a negative status before any launch: a negative count, a count >= 2^31, a null pointer with a non-zero count
 * (colors may be null), mean_len not positive and finite, q_bits outside [1, 40] or with F * 2^q_bits > 2^59, max_cost negative
 * or NaN.  A zero count skips the launches over it. */
int dgs_decimate_quadrics(long long n_vertices, const float* pos, long long n_faces, const int* faces, float mean_len, int q_bits,
                          long long* rows, void* stream);

int dgs_decimate_edges(long long n_vertices, const float* pos, const long long* rows, const unsigned char* flags, long long n_faces,
                       const int* faces, long long n_edges, const int* edges, const long long* adj_offsets, const int* adj, long long n_adj,
                       const long long* vf_offsets, const int* vf, long long n_vf, int q_bits, float max_cost, float* cost, float* place,
                       unsigned char* valid, void* stream);

int dgs_decimate_select(long long n_vertices, long long n_edges, const int* edges, const float* cost, const unsigned char* compete,
                        unsigned long long* m1, unsigned long long* m2, unsigned char* selected, void* stream);

int dgs_decimate_apply(long long n_vertices, float* pos, long long* rows, float* colors, const unsigned char* flags, unsigned char* moved,
                       int* vmap, long long n_edges, const int* edges, const float* place, long long n_sel, const int* sel, long long n_faces,
                       int* faces, unsigned char* keep, void* stream);

/* out = {threads per workgroup, items per thread, the largest Q, the budget 59 of Q + ceil(log2 F), W_MAX, the exponent of lambda
 *        (-10), the least valence of an interior opposite vertex, the fixed-point bits of mean_len}: a workgroup takes out[0] * out[1]
 *        faces, edges or vertices. */
int dgs_decimate_layout(int out[8]);

/* Mesh hole filling: the list ranking behind dgs_amd/mesh_fill.py: boundary_loops and the loop sums, smoothed rims and ring emission
 * behind fill_holes (the role trimesh's fill_holes has at the end of the reference's clean_mesh, render_mesh_trajectory.py:41-88 --
 * which closes 3- and 4-edge loops only; this one closes every simple loop up to a size the caller chooses).  Version 2 libraries
 * from this commit on also carry the dgs_fill_* calls; the version number is unchanged because nothing that existed before changes
 * (the precedent of dgs_tri_*).  THE STATEMENT -- every fp operation rounded on its own (-ffp-contract=off), fp64 unless it says
 * otherwise; rn() is round-to-nearest-even to an integer; an int64 is converted to fp64 by one rounding; dgs_amd/mesh_fill.py states
 * the same arithmetic in PyTorch and CPU tensors run it: the results are bit-identical.
 *
 * 1. LOOPS (the wrapper: one sort of packed 64-bit keys, run lengths and prefix sums on the tensors' device; dgs_cc_labels).  Faces
 *    that name a vertex twice take no part.  A half-edge (a -> b) is a BOUNDARY half-edge when the undirected edge {a, b} occurs
 *    exactly once among all half-edges; a vertex is SIMPLE when exactly one boundary half-edge leaves it and exactly one enters it; a
 *    HOLE is a closed cycle of boundary half-edges over simple vertices (a cycle through a bow-tie vertex and an open chain are not).
 *    The boundary half-edges are the NODES, numbered in ascending order of their tail vertex; succ[h] is the node whose tail is the
 *    head of h, if that head is simple.  dgs_cc_labels on the pairs (h, succ[h]) gives every node the smallest node of its list --
 *    of a cycle, the half-edge that leaves its smallest vertex: the LEADER.  A list is a cycle iff every node of it has a successor.
 * 2. RANKS (dgs_fill_rank).  leader[h] is the leader of h's cycle if the cycle is to be ranked (closed, 3 <= n <= max_hole_edges),
 *    else -1.  The cycle is cut in front of its leader and ranked by pointer jumping on packed entries next << 32 | distance:
 *      init      E[h] = (h, 0) if leader[h] < 0, succ[h] is outside [0, n_nodes) or succ[h] == leader[h] (the end of a list),
 *                else (succ[h], 1)
 *      a round   with (x, d) = E[h] and (y, e) = E[x]:  E'[h] = (y, d + e) -- one load gives both; a round reads one buffer and
 *                writes the other, ONE LAUNCH PER ROUND, n_rounds of them; an end (x == h, d == 0) stays what it is
 *      ranks     rank[h] = -1 if leader[h] < 0, 0 if h == leader[h], else distance + 1
 *    n_rounds = ceil(log2(longest ranked cycle)) is the caller's: after r rounds a node has jumped min(2^r, its distance to the end).
 *    rank is the position in HOLE ORDER, the reverse of the boundary direction, starting at the cycle's smallest vertex: a filler
 *    triangle (r_i, r_i+1, x) then has the winding of the mesh.  No kernel waits for another workgroup and none walks a list: a
 *    malformed successor table (a cycle that is never cut, two nodes with one successor) gives wrong ranks after the same n_rounds
 *    launches, never a hang.  The result lies in buf_a after an even number of rounds and in buf_b after an odd one.
 * 3. LAYOUT (the wrapper).  The rims of the loops to fill, concatenated in hole order: loop_vertices [B] int32, loop_offsets [L + 1]
 *    int64, rim_loop [B] int32 (the loop of every slot).  A loop of n = 3 gets one triangle and no vertex.  Otherwise
 *    R = max(1, (113 n + 355) / 710) rings (n / 2 pi in integers: rings about one rim edge apart; R = 1 up to n = 9): ring 1 has n
 *    vertices, ring k (2 <= k < R) has m_k = (n (R - k) + R / 2) / R, ring R is one vertex, the centre; with R = 1 the centre is
 *    all.  rings [n_rings,10] int32, one row per ring in (loop, k) order: loop, k, R, n, vertices of the ring, id of its first
 *    vertex, vertices of the ring before it (the rim for k = 1), id of that ring's first vertex (-1: the rim), index of the first
 *    face of the strip between the two among the new faces, faces of the strip (a loop of 3: one row, no vertex, one face).
 *    vert_ring [n_new] and face_ring [n_new_faces] int32 name the row of every new vertex and face.  New vertices and faces follow
 *    the input's, loop by loop, ring by ring, strip by strip.
 * 4. FRAME.  centre = (min + max) * 0.5 per axis (fp32) and scale = 2^-e as in dgs_decimate (step 0 there);
 *    P(v) = (fp64(v) - fp64(centre)) * scale, |P_i| <= 1 + 2^-22.  Colours enter as C = fp64(clamp(colour, 0, 1)), a NaN as 0.
 * 5. RIM (dgs_fill_rim, a thread per rim slot).  With i the slot's index in its loop of n and all indices mod n:
 *      S_i = sum over d = -4 .. 4, IN THIS ORDER, of w_d P(r_i+d), w = (1, 8, 28, 56, 70, 56, 28, 8, 1) / 256: the rim after four
 *      passes of the cyclic [1/4 1/2 1/4] filter (acc = w_-4 P; acc = acc + w_-3 P; ...); SC_i the same of C.  The rim itself
 *      never moves; S only shapes the new rings.
 *      rows [n_loops,16] int64 (cleared by the call), columns 0..2 sum of rn(P(r_i) 2^30); 3..5 the Newell sum, component a with
 *      (b, c) the next two axes: sum of rn(((P_b(r_i) - P_b(r_i+1)) * (P_c(r_i) + P_c(r_i+1))) 2^28); 6..8 sum of rn(C(r_i) 2^24).
 *    Integer sums: their order and grouping cannot change a bit (the kernel sums neighbouring slots of a loop on chip, as
 *    dgs_simplify_accumulate does).  NO SUM CAN OVERFLOW for n_rim < 2^31: a position term is below 2^30.001, a Newell term below
 *    (2.000001)^2 2^28 < 2^30.001, a colour term at most 2^24; 2^31 of them stay below 2^62.
 * 6. VERTICES (dgs_fill_emit, a thread per new vertex).  Vertex j of ring k with m vertices in a loop of n:
 *      c = fp64(row_a) / (fp64(n) * 2^30) per axis;  u = 1 - fp64(k) / fp64(R)
 *      i0 = (j n) / m, t = fp64((j n) mod m) / fp64(m);  s = S_i0 + t * (S_i0+1 - S_i0);  y = c + u * (s - c);  ring R: y = c
 *      vertex = fp32(fp64(centre) + y * (1 / scale));  colour = fp32(cc + u * (sc - cc)) with cc = fp64(row_6+a) / (fp64(n) * 2^24)
 *      and sc from SC as s from S.
 * 7. FACES (dgs_fill_emit, a thread per new face, after the vertices).  A loop of 3: (r_0, r_1, r_2).  The strip into ring R (the
 *    fan): (A_e, A_e+1 mod m, centre) for every edge e of the ring before it (the rim if R = 1).  The strip rim -> ring 1 (R > 1),
 *    two faces per rim edge i, with q the ring: the quad r_i, r_i+1, q_i+1, q_i is split along r_i - q_i+1 into (r_i, r_i+1, q_i+1),
 *    (r_i, q_i+1, q_i), or along r_i+1 - q_i into (r_i, r_i+1, q_i), (r_i+1, q_i+1, q_i): with area(a, b, c) = ((b - a) x (c - a)) . N
 *    on the fp32 output positions converted to fp64, N = fp64 of the Newell sum, the second split is taken iff the smaller of its
 *    two areas is greater than the smaller of the first's (a tie or a NaN takes the first).  The strip ring k - 1 (A, m vertices)
 *    -> ring k (B, m' vertices), 2 <= k < R, is the merge of the two sequences by parameter in closed form: outer edge i gives
 *    (A_i, A_i+1 mod m, B_g), g = ((i + 1) m' - 1) / m; inner edge j gives (A_h, B_j+1 mod m', B_j), h = ((j + 1) m / m') mod m; the
 *    m outer faces come first.
 *
 * Arguments.  All device memory.  succ, leader, rank [n_nodes] int32; buf_a, buf_b [n_nodes] 64-bit words, two different buffers.
 * vertices [n_vertices,3] fp32, colors likewise or NULL (then SC and colors_out are NULL too); S, SC [n_rim,3] fp64; rows
 * [n_loops,16] int64; vertices_out [n_old + n_new,3] fp32 whose first n_old rows hold the input vertices (the face kernel reads them)
 * and colors_out likewise; faces_out [n_new_faces,3] int32.  dgs_fill_rank: n_rounds + 2 launches; dgs_fill_rim: the clear and one
 * launch; dgs_fill_emit: two launches.
 * GUARDS.  Every id and offset read from a buffer is range-checked before an address is formed from it: a rim slot whose loop, range
 * or vertex ids are out of range writes zeros and adds nothing; a new vertex or face whose ring row, loop or index is out of range
 * is written as zeros; the face (0, 0, 0).  The Python wrapper produces no such input.
 * Refused with a negative status before any launch: a negative count, a count >= 2^31 (n_old + n_new among them), n_rounds outside
 * [0, 31], buf_a == buf_b, a null pointer with a non-zero count (colors / SC / colors_out may be null, together), a centre that is
 * not finite, a scale that is not positive and finite, new vertices or faces without rings, loops or a rim.  A zero count skips
 * the launches over it. */
int dgs_fill_rank(long long n_nodes, const int* succ, const int* leader, int n_rounds, unsigned long long* buf_a, unsigned long long* buf_b,
                  int* rank, void* stream);

int dgs_fill_rim(long long n_vertices, const float* vertices, const float* colors, long long n_rim, const int* loop_vertices,
                 const int* rim_loop, long long n_loops, const long long* loop_offsets, double centre_x, double centre_y, double centre_z,
                 double scale, double* S, double* SC, long long* rows, void* stream);

int dgs_fill_emit(long long n_old, long long n_new, const int* vert_ring, long long n_new_faces, const int* face_ring, long long n_rings,
                  const int* rings, long long n_loops, const long long* loop_offsets, long long n_rim, const int* loop_vertices,
                  const long long* rows, const double* S, const double* SC, double centre_x, double centre_y, double centre_z, double scale,
                  float* vertices_out, float* colors_out, int* faces_out, void* stream);

/* out = {threads per workgroup (T: a workgroup takes T nodes, rim slots, vertices or faces), items per thread, the fixed-point bits
 *        of the position sums, of the Newell sums and of the colour sums, the columns of a ring row, the taps of the smoothed rim,
 *        the largest n_rounds}. */
int dgs_fill_layout(int out[8]);

#ifdef __cplusplus
}
#endif
#endif
