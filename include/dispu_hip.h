/*
 * dispu_hip.h -- C ABI of libdispu_hip.so, the MI355X (gfx950) implementation of the Dis-PU
 * point-sampling / grouping / distance hot path.
 *
 * This is the drop-in boundary: every entry point below replaces one plain-pointer "Launcher"
 * that the reference's TensorFlow op kernels call from Compute() (or, for the three CPU-only
 * ops and the nanoflann k-NN, the CPU function itself).  The reference interface each one
 * replaces is cited as file:line in the upstream tree (liruihui/Dis-PU).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / TF types.
 *   - every pointer is a DEVICE pointer owned by the caller; the library never allocates.
 *     Scratch is passed in; `*_scratch_bytes` tells how much an op needs (0 = none).
 *   - row-major fp32 data, int32 indices; clouds are AoS [b, n, 3].
 *   - the last argument is the hipStream_t to launch on (as void*; NULL = default stream);
 *     launches are asynchronous w.r.t. the host, exactly like the reference launchers.
 *   - return value: 0 (hipSuccess) or the hipError_t code of the failing call.  The reference
 *     launchers return void and never check errors (tf_sampling_g.cu:194-211).
 *   - gradient entry points zero-fill their outputs first (the reference ops do the memset
 *     before calling the launcher: tf_sampling.cpp:174, tf_grouping.cpp:208,
 *     tf_nndistance_g.cu:153-154).
 *   - `arith` selects the pinned floating-point flavour of d2 = dx*dx + dy*dy + dz*dz:
 *       DISPU_ARITH_PLAIN    ((dx*dx + dy*dy) + dz*dz)             the reference's CPU functions
 *       DISPU_ARITH_CONTRACT fmaf(dz,dz, fmaf(dx,dx, dy*dy))       nvcc-contracted GPU kernels
 *     Index results are identical between the two except on near-ties.
 */
#ifndef DISPU_HIP_H
#define DISPU_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DISPU_ARITH_PLAIN 0
#define DISPU_ARITH_CONTRACT 1
/* OR-able with the above, dispu_approx_match only: evaluate exp() with a bit-reproducible fmaf-chain
 * polynomial instead of the hardware v_exp_f32 (the reference uses the hardware __expf).  Parity/debug
 * mode: results are then bit-identical to oracle/dispu_oracle.c; about 1.6x slower. */
#define DISPU_ARITH_PINNED_EXP 2
/* OR-able, dispu_knn_xyz only: force the lane-per-query kernel instead of the wave-per-query fast path that is
 * used for n <= 1024 (identical results; A/B tests and profiling). */
#define DISPU_KNN_LANE_PER_QUERY 4
/* OR-able, dispu_point_to_mesh only: visit every face tile instead of culling tiles by their boxes (identical results; A/B tests). */
#define DISPU_MESH_BRUTE_FORCE 8
/* faces per tile of dispu_point_to_mesh's face layout */
#define DISPU_MESH_TILE 64

/* Library / ABI version.  1 = round 1.  2 = round 2: the *_ws k-NN entries, dispu_attention_project, the bf16 GEMMs (and a
 * scratch argument inserted into dispu_match_cost(_grad) under the same names -- an in-place signature change, withdrawn in 3).
 * 3 = round 3: dispu_match_cost / dispu_match_cost_grad are the reference's launcher signatures again (as in version 1, no
 * scratch) and the scratch-taking fast paths are dispu_match_cost_ws / dispu_match_cost_grad_ws; dispu_fps_ws (scratch with an
 * explicit size), dispu_prob_sample, dispu_selection_sort; the fused training kernels.  A symbol never changes signature again:
 * new forms get new names.  4 = round 4: additions only (dispu_attention_fwd_lse / dispu_attention_bwd, ...).
 * 5 = round 6: dispu_approx_match works inside the reference op's own temp ([b, 2(n+m)] floats; until 4 it needed
 * dispu_approx_match_scratch_bytes and had no way to refuse less); the tiled fast path is dispu_approx_match_ws with an explicit size.
 * Still 5 with the evaluator's mesh metrics (dispu_point_to_mesh, dispu_disk_*, dispu_row_mean_std) and its geodesic disks
 * (dispu_geodesic_*), the ragged-batch entries (dispu_fps_segments, dispu_knn_patch_segments, dispu_normalize_segments) and the
 * mesh sampler (dispu_mesh_sample, dispu_poisson_disk_*, dispu_sort_rows_i32), and the large-cloud sampling (dispu_fps_cells*,
 * dispu_fps_segments_auto*), and the oriented normals (dispu_pca_normals_*), and the outlier filters (dispu_knn_mean_dist_*,
 * dispu_radius_count_*, dispu_outlier_threshold_segments, dispu_compact_*), and the cross-cloud search with the attribute transfer
 * (dispu_knn_cross_*, dispu_transfer_attributes_segments), and the consistent orientation (dispu_orient_consistent_*), and the
 * moving-least-squares projection (dispu_mls_project_*), and the surface reconstruction (dispu_signed_distance_*, dispu_lattice_*,
 * dispu_contour_*), and the clustering (dispu_cluster_*): additions only. */
int dispu_version(void);
/* Stream / event / memset operations on raw HIP handles (hipEventRecord, hipStreamWaitEvent, hipMemsetAsync): what a host that
 * re-issues a recorded launch sequence needs beside the kernels (dis-pu_amd/_lib.py:Tape; no reference counterpart: TF's executor). */
int dispu_event_record(void* event, void* stream);
int dispu_stream_wait_event(void* stream, void* event);
int dispu_memset_async(void* dst, int value, size_t bytes, void* stream);
/* hipGetErrorString for the codes returned below. */
const char* dispu_error_string(int code);

/* ---- tf_ops/sampling ------------------------------------------------------------------------ */

/* farthestpointsamplingLauncher(b,n,m,inp,temp,out)   tf_ops/sampling/tf_sampling.cpp:94,118;
 * kernel tf_sampling_g.cu:105-170.  out[b,m] int32; out[:,0] = 0.
 * dispu_fps keeps the reference launcher's contract for `temp`: the op allocates it as {32, n} floats whatever b is
 * (tf_sampling.cpp:115), so this entry never touches more than min(b,32)*n floats of it -- batches above 32 clouds run as
 * consecutive groups of 32 on the stream.  temp may be NULL for n <= 24576 (the dense register kernels need none).
 * dispu_fps_ws is the same op with the scratch size stated: `temp_bytes` >= dispu_fps_scratch_bytes(b,n,m) (= 4*b*n for
 * 4096 < n <= 24576 with m >= 64: the Morton-sorted permutation of the region-skipping kernels, csrc/fps_wave.hip; and for
 * n > 24576: the running distances) selects the fastest kernel; with less (or NULL) the dense kernels answer (n <= 24576)
 * with identical results, and n > 24576 is refused (hipErrorInvalidValue) instead of writing out of bounds. */
size_t dispu_fps_scratch_bytes(int b, int n, int m);
int dispu_fps(int b, int n, int m, const float* inp, float* temp, int* out, int arith, void* stream);
int dispu_fps_ws(int b, int n, int m, const float* inp, float* temp, size_t temp_bytes, int* out, int arith, void* stream);
/* A ragged batch of C clouds, the sampling of DisPU/model.py:315-323 and :375 (farthest_point_sample over each whole cloud) for
 * clouds of different sizes in one call.  inp [sum n_c, 3] packs the clouds; off [C+1] (device int32, off[0] = 0) holds the
 * segment offsets, segment c samples m_c = moff[c+1] - moff[c] >= 1 points into out[moff[c] ..] (local indices, out[moff[c]] = 0).
 * off_host / moff_host are the same offsets in host memory: they choose the kernels and LDS sizes and are never read on the
 * device.  Every segment's indices are bit-identical to dispu_fps_ws on that cloud alone, in both arithmetic flavours.  Segments
 * go to the family dispu_fps_ws would pick (register kernels; region-skipping kernels for 4096 < n_c <= 24576 with m_c >= 64;
 * the streaming kernel above 24576), one launch per family sized for its largest segment; several families run concurrently
 * on side streams joined back to `stream` by events.  temp_bytes >= dispu_fps_segments_scratch_bytes(C, off_host, moff_host)
 * (4 * sum n_c when a segment needs the permutation or the running distances, else 0). */
size_t dispu_fps_segments_scratch_bytes(int C, const int* off_host, const int* moff_host);
int dispu_fps_segments(int C, const int* off, const int* moff, const int* off_host, const int* moff_host, const float* inp, void* temp,
                       size_t temp_bytes, int* out, int arith, void* stream);
/* The same sampling (tf_sampling.cpp:94,118; kernel tf_sampling_g.cu:105-170) for LARGE clouds, csrc/fps_cells.hip (pre-pass: csrc/morton_cells.hip): the cloud stays in
 * global memory, a device-wide pre-pass (bounding boxes, Morton keys, one dispu_radix_sort_pairs over the batch, cells of S consecutive
 * sorted positions with their boxes) lets every round skip the cells whose box is farther from the new sample than their largest
 * running distance.  The indices are those of dispu_fps_ws and dispu_fps_segments bit for bit, in both arithmetic flavours: skipped
 * updates are no-ops, ties are decided by the original index (k mod 512, then k).
 * dispu_fps_cells takes a ragged batch described as in dispu_fps_segments and serves EVERY segment with these kernels, for any
 * n_c >= 1 and m_c >= 1 (m_c > n_c included) up to n_c = 2^24; the offsets need C <= 65535.  cell: 0 = the cell size the dispatch
 * picks (64 up to 262144 points, doubling above: at most 4096 cells per segment), or a power of two in 64 .. 4096 to force that size
 * on every segment for which it is not smaller than the automatic one (tests visit every size at small n).  status [C] (device):
 * 0, or 1 for a segment that holds a non-finite coordinate, for which NO index is written.  scratch: 16-byte aligned,
 * scratch_bytes >= dispu_fps_cells_scratch_bytes(C, off_host, moff_host, cell) (0 for illegal offsets, cell sizes or segments above
 * 2^24 points); a scratch that is NULL or too small is refused (hipErrorInvalidValue) untouched.
 * dispu_fps_cells_wanted(n, m): 1 where the cell kernels beat the streaming kernel (measured: profiles/fps_large_bench.json), never
 * for n <= 24576. */
size_t dispu_fps_cells_scratch_bytes(int C, const int* off_host, const int* moff_host, int cell);
int dispu_fps_cells(int C, const int* off, const int* moff, const int* off_host, const int* moff_host, const float* inp, void* scratch,
                    size_t scratch_bytes, int* out, int* status, int arith, int cell, void* stream);
int dispu_fps_cells_wanted(int n, int m);
/* dispu_fps_segments (tf_sampling.cpp:94,118; tf_sampling_g.cu:105-170 per segment) with a fourth family: segments with n_c > 24576 for
 * which dispu_fps_cells_wanted(n_c, m_c) says yes go through the cell kernels, all others through the launchers of dispu_fps_segments,
 * concurrently on side streams.  Same arguments and results; in addition status [C] (device; may be NULL when no segment is wanted by
 * the cell kernels) is 0, or 1 for a cell-kernel segment with a non-finite coordinate, whose indices are then NOT written: sample
 * it again with dispu_fps_segments.  temp: 16-byte aligned, temp_bytes >= dispu_fps_segments_auto_scratch_bytes(C, off_host, moff_host). */
size_t dispu_fps_segments_auto_scratch_bytes(int C, const int* off_host, const int* moff_host);
int dispu_fps_segments_auto(int C, const int* off, const int* moff, const int* off_host, const int* moff_host, const float* inp, void* temp,
                            size_t temp_bytes, int* out, int* status, int arith, void* stream);

/* probsampleLauncher(b,n,m,inp_p,inp_r,temp,out)   tf_sampling.cpp:65,83-89; kernels tf_sampling_g.cu:7-104 (cumulative sums
 * of the weights inp_p[b,n] into temp[b,n], then out[b,m] = the first position whose cumulative weight is >= inp_r * total).
 * Optional op of the reference (never called by the shipped graph).  The association of the sums is the reference's. */
int dispu_prob_sample(int b, int n, int m, const float* inp_p, const float* inp_r, float* temp, int* out, void* stream);

/* gatherpointLauncher(b,n,m,inp,idx,out)   tf_sampling.cpp:125; kernel tf_sampling_g.cu:172-181. */
int dispu_gather_point(int b, int n, int m, const float* inp, const int* idx, float* out, void* stream);

/* scatteraddpointLauncher(b,n,m,out_g,idx,inp_g)   tf_sampling.cpp:150,174; kernel :183-192. */
int dispu_gather_point_grad(int b, int n, int m, const float* out_g, const int* idx, float* inp_g, void* stream);

/* ---- tf_ops/grouping ------------------------------------------------------------------------ */

/* queryBallPointLauncher(b,n,m,radius,nsample,xyz1,xyz2,idx,pts_cnt)   tf_ops/grouping/tf_grouping.cpp:67;
 * kernel tf_grouping_g.cu:3-36.  radius is a device pointer; only radius[0] is read.  Rows of idx
 * whose query has no neighbour are left untouched (reference behaviour). */
int dispu_query_ball(int b, int n, int m, const float* radius, int nsample, const float* xyz1, const float* xyz2,
                     int* idx, int* pts_cnt, int arith, void* stream);

/* groupPointLauncher(b,n,c,m,nsample,points,idx,out)   tf_grouping.cpp:146; kernel tf_grouping_g.cu:40-57. */
int dispu_group_point(int b, int n, int c, int m, int nsample, const float* points, const int* idx, float* out,
                      void* stream);

/* groupPointGradLauncher(b,n,c,m,nsample,grad_out,idx,grad_points)   tf_grouping.cpp:177,208; kernel :61-78. */
int dispu_group_point_grad(int b, int n, int c, int m, int nsample, const float* grad_out, const int* idx,
                           float* grad_points, void* stream);

/* selectionSortLauncher(b,n,m,k,dist,outi,out)   tf_grouping.cpp:112,141; kernel tf_grouping_g.cu:83-123.  dist/outi/out [b,m,n]:
 * out is a copy of dist whose first k entries per row are the k smallest in ascending order (k rounds of selection sort: swap
 * position s with the FIRST minimum of positions s..n-1), outi the matching positions.  Optional op of the reference. */
int dispu_selection_sort(int b, int n, int m, int k, const float* dist, int* outi, float* out, void* stream);

/* tf_grouping.knn_point(k, xyz1[b,n,c], xyz2[b,m,c]) -> (val = -d2 [b,m,k], idx [b,m,k])
 * tf_ops/grouping/tf_grouping.py:116-141 (pure TF: broadcast-subtract, reduce_sum, top_k).  Any k <= n, c up to 4096 (k <= 32 and c <= 128: register-resident
 * kernels; beyond: the radix-select kernel of csrc/knn_general.hip, k <= 4096). */
int dispu_knn_point(int b, int n, int m, int c, int k, const float* xyz1, const float* xyz2, float* val, int* idx,
                    void* stream);

/* tf_grouping.knn_point_2(k, points[b,n,c], queries[b,m,c]) -> (dist [b,m,k] = +D, idx [b,m,k])
 * tf_grouping.py:61-66,95-114 (D = rA - 2 A.B^T + rB; top_k(-D)).  The (batch,point) pair tensor of
 * the reference is assembled by the Python shim.  dist may be NULL.  Limits as dispu_knn_point. */
int dispu_knn_feat(int b, int n, int m, int c, int k, const float* points, const float* queries, float* dist,
                   int* idx, void* stream);

/* dispu_knn_feat with explicit row strides (in floats) so points/queries can be column slices of a wider buffer. */
int dispu_knn_feat_strided(int b, int n, int m, int c, int k, const float* points, int ldp, const float* queries,
                           int ldq, float* dist, int* idx, void* stream);
/* dispu_knn_feat_strided with caller scratch (dispu_knn_feat_scratch_bytes(b,n,m,c,k) bytes, 0 = this shape needs none): clouds of
 * 513 .. 4096 points, c <= 64, k <= 32 are searched in chunks of <= 256 candidates by the wave-per-query kernel and merged.
 * Clouds of 513 .. 1024 points with c <= 48 (the dense blocks of the second 16x pass) take ONE pass instead and leave the scratch
 * untouched (both entries; dispu_knn_feat_strided needs no scratch for them either).  Same results. */
size_t dispu_knn_feat_scratch_bytes(int b, int n, int m, int c, int k);
int dispu_knn_feat_strided_ws(int b, int n, int m, int c, int k, const float* points, int ldp, const float* queries, int ldq,
                              float* dist, int* idx, void* scratch, size_t scratch_bytes, void* stream);

/* ---- libs/nearest_neighbors ----------------------------------------------------------------- */

/* cpp_knn_batch_omp(batch_data,batch_size,npts,dim=3,queries,nqueries,K,indices)
 * libs/nearest_neighbors/knn_.cxx:104-135 (nanoflann KD-tree on the host, int64 output).  Device-side
 * exact brute force; idx int32 [b,m,k] ascending distance, ties -> lower index; dist (squared, may be
 * NULL).  k <= n, k <= 4096 (k > 32: csrc/knn_general.hip). */
int dispu_knn_xyz(int b, int n, int m, int k, const float* support, const float* query, int* idx, float* dist,
                  int arith, void* stream);
/* The same search with caller scratch (dispu_knn_xyz_scratch_bytes(b,n,m,k) bytes; 0 = this shape needs none): clouds of
 * 1025 .. 8192 points and k <= 32 are cut into chunks of <= 1024 candidates, searched by the wave-per-query kernel and merged
 * (2x faster than the lane-per-query kernel at (32, 4096, 4096, 16), the second pass of 16x upsampling).  Same results. */
size_t dispu_knn_xyz_scratch_bytes(int b, int n, int m, int k);
int dispu_knn_xyz_ws(int b, int n, int m, int k, const float* support, const float* query, int* idx, float* dist, void* scratch,
                     size_t scratch_bytes, int arith, void* stream);

/* ---- tf_ops/interpolation (CPU-only ops in the reference) ------------------------------------- */

/* threenn_cpu(b,n,m,xyz1,xyz2,dist,idx)   tf_ops/interpolation/tf_interpolate.cpp:60-103. */
int dispu_three_nn(int b, int n, int m, const float* xyz1, const float* xyz2, float* dist, int* idx, int arith,
                   void* stream);
/* threeinterpolate_cpu(b,m,c,n,points,idx,weight,out)   tf_interpolate.cpp:107-127. */
int dispu_three_interpolate(int b, int m, int c, int n, const float* points, const int* idx, const float* weight,
                            float* out, void* stream);
/* threeinterpolate_grad_cpu(b,n,c,m,grad_out,idx,weight,grad_points)   tf_interpolate.cpp:131-153. */
int dispu_three_interpolate_grad(int b, int n, int c, int m, const float* grad_out, const int* idx,
                                 const float* weight, float* grad_points, void* stream);

/* ---- tf_ops/nn_distance --------------------------------------------------------------------- */

/* NmDistanceKernelLauncher(b,n,xyz,m,xyz2,result,result_i,result2,result2_i)
 * tf_ops/nn_distance/tf_nndistance.cpp:168; kernel tf_nndistance_g.cu:5-131. */
int dispu_nn_distance(int b, int n, const float* xyz1, int m, const float* xyz2, float* dist1, int* idx1, float* dist2,
                      int* idx2, int arith, void* stream);
/* NmDistanceGradKernelLauncher(b,n,xyz1,m,xyz2,grad_dist1,idx1,grad_dist2,idx2,grad_xyz1,grad_xyz2)
 * tf_nndistance.cpp:208; kernel tf_nndistance_g.cu:132-157. */
int dispu_nn_distance_grad(int b, int n, const float* xyz1, int m, const float* xyz2, const float* grad_dist1,
                           const int* idx1, const float* grad_dist2, const int* idx2, float* grad_xyz1,
                           float* grad_xyz2, void* stream);

/* ---- tf_ops/approxmatch --------------------------------------------------------------------- */

/* approxmatchLauncher(b,n,m,xyz1,xyz2,match,temp)   tf_ops/approxmatch/tf_approxmatch.cpp:141,164-170;
 * kernel tf_approxmatch_g.cu:1-182.  match [b,m,n].
 * dispu_approx_match: the launcher's own contract -- `temp` is the op's [b, 2*(n+m)] float allocation
 * (tf_approxmatch.cpp:164-170) and nothing behind it is written.  One workgroup per cloud like the reference's kernel, every sum in
 * the reference's sequential order (bit-exact to oracle/dispu_oracle.c:orc_approx_match with DISPU_ARITH_PINNED_EXP); slow.
 * dispu_approx_match_ws: the fast path (2-D tiled passes, csrc/approxmatch.hip).  `temp`: dispu_approx_match_scratch_bytes(b,n,m)
 * bytes -- the per-level ratio vectors and the per-chunk partial sums; `temp_bytes` is what the caller really allocated and a smaller
 * scratch is refused (hipErrorInvalidValue) without being touched.  Sums are associated in chunks of 128 partners (oracle chunk = 128). */
size_t dispu_approx_match_scratch_bytes(int b, int n, int m);
int dispu_approx_match(int b, int n, int m, const float* xyz1, const float* xyz2, float* match, float* temp, int arith,
                       void* stream);
int dispu_approx_match_ws(int b, int n, int m, const float* xyz1, const float* xyz2, float* match, float* temp,
                          size_t temp_bytes, int arith, void* stream);
/* dispu_approx_match_ws without its last launch (the assembly of `match`): init, the ten column passes and the 1 + 9 row passes of the
 * auction (tf_approxmatch_g.cu:50-160).  `temp` / `temp_bytes` and every refusal as dispu_approx_match_ws; afterwards `temp` holds the ten
 * (ratioL, ratioR) vector pairs and pass 2's partial sums of the last level, byte for byte what dispu_approx_match_ws leaves there. */
int dispu_approx_match_levels_ws(int b, int n, int m, const float* xyz1, const float* xyz2, float* temp, size_t temp_bytes, int arith,
                                 void* stream);
/* The EMD term of the training loss, `10.0 * earth_mover(fine, gt, radius)` (DisPU/model.py:77; loss_utils.py:170-176), value and
 * gradient without a [b, m, n] `match`: replaces approxmatchLauncher's `match += w` (tf_approxmatch_g.cu:152), matchcost (:183-225) and
 * matchcostgrad1 (:270-291) behind one entry.  xyz1 [b, n, 3] = the prediction, xyz2 [b, m, 3] = the ground truth, `temp` = the scratch
 * dispu_approx_match_levels_ws(b, n, m, xyz1, xyz2, ...) filled in the same `arith` mode.  Every plan entry match[l][k] =
 * sum_t exp(level_t d2) ratioL_t[k] ratioR_t[l] is rebuilt in registers in dispu_approx_match_ws's order and feeds
 *   cost [b]          = sum_{k,l} sqrt(d2) match[l][k]                                   (written, not scaled)
 *   dpred [b, n, 3]  += (coef / radius[b]) * sum_l match[l][k] (xyz1_k - xyz2_l) rsqrt(max(d2, 1e-20))     (radius NULL: factor coef)
 * approx_match carries no gradient (tf_approxmatch.py:22), so this is the whole gradient of the term w.r.t. xyz1.  n != m allowed.
 * Two launches (tiles, combine); partial sums are combined in ascending tile order, no float atomics: run-to-run identical.
 * `scratch`: dispu_emd_loss_grad_scratch_bytes(b, n, m) = 4 * b * (nc * n * 3 + ceil(n / 256) * nc) bytes, nc = ceil(m / ch), where
 * ch = 128 is halved while ch > 32 and ceil(n / 256) * ceil(m / ch) * b < 1024.  b < 0, n or m < 1, a NULL pointer (radius excepted)
 * or scratch_bytes below that: hipErrorInvalidValue, nothing written; b == 0 returns 0 without a launch. */
size_t dispu_emd_loss_grad_scratch_bytes(int b, int n, int m);
int dispu_emd_loss_grad(int b, int n, int m, const float* xyz1, const float* xyz2, float* temp, const float* radius, float coef,
                        float* cost, float* dpred, float* scratch, size_t scratch_bytes, int arith, void* stream);
/* matchcostLauncher(b,n,m,xyz1,xyz2,match,out)   tf_approxmatch.cpp:142; kernel tf_approxmatch_g.cu:183-228.
 * dispu_match_cost: the launcher's own signature, no scratch (one workgroup per cloud, like the reference's kernel).
 * dispu_match_cost_ws: the fast path; `scratch`: dispu_match_cost_scratch_bytes(b,n,m) bytes (one partial per tile of `match`).
 * The two differ in the association of the sum only (both within 1e-5 of the reference's). */
int dispu_match_cost(int b, int n, int m, const float* xyz1, const float* xyz2, const float* match, float* cost, int arith,
                     void* stream);
size_t dispu_match_cost_scratch_bytes(int b, int n, int m);
int dispu_match_cost_ws(int b, int n, int m, const float* xyz1, const float* xyz2, const float* match, float* cost,
                        float* scratch, int arith, void* stream);
/* matchcostgradLauncher(b,n,m,xyz1,xyz2,match,grad1,grad2)   tf_approxmatch.cpp:143; kernels :229-295.
 * dispu_match_cost_grad: the launcher's signature, no scratch.  dispu_match_cost_grad_ws: grad1 as partial sums per chunk of
 * cloud-2 points (`scratch`: dispu_match_cost_grad_scratch_bytes(b,n,m) bytes), more workgroups for small b. */
int dispu_match_cost_grad(int b, int n, int m, const float* xyz1, const float* xyz2, const float* match, float* grad1,
                          float* grad2, int arith, void* stream);
size_t dispu_match_cost_grad_scratch_bytes(int b, int n, int m);
int dispu_match_cost_grad_ws(int b, int n, int m, const float* xyz1, const float* xyz2, const float* match, float* grad1,
                             float* grad2, float* scratch, int arith, void* stream);

/* ---- per-point MLP stacks (Common/tf_util.py conv1d/conv2d 1x1, Common/ops.py blocks) --------------
 * The reference builds these from TensorFlow core ops (conv2d -> bias_add -> relu, matmul, softmax,
 * gather_nd, concat); there is no native launcher to replace, so each entry point cites the Python block
 * whose arithmetic it implements.  Matrices are (pointer, row stride `ld*` in floats[, batch stride `s*`]). */

/* Y[z][m,n] = R2 + R1 + act( sum_k X[z][m,k] * W[z][k,n] + bias[n] ), k ascending, fp32 MFMA (bit-equal to an
 * fmaf chain).  transb != 0: W is given as [n][k].  act: 0 none, 1 ReLU.  bias/R1/R2 may be NULL.
 * conv1d/conv2d with 1x1 kernels: Common/tf_util.py:52-115,120-185; tf.matmul of PointNonLocalCell ops.py:326,339. */
int dispu_linear(int batch, int M, int K, int N, const float* X, long ldx, long sx, const float* W, long ldw, long sw,
                 int transb, const float* bias, int act, float* Y, long ldy, long sy, const float* R1, long ldr1,
                 long sr1, const float* R2, long ldr2, long sr2, void* stream);
/* dispu_linear with an inference-BatchNorm epilogue (tf_util.py:176-185: conv -> bias_add -> batch_norm -> relu):
 * Y = R2 + R1 + act( (X.W + bias) * scale[n] + shift[n] ); scale/shift are the folded BN (gamma/sqrt(var+eps), ...). */
int dispu_linear_bn(int batch, int M, int K, int N, const float* X, long ldx, long sx, const float* W, long ldw, long sw,
                    int transb, const float* bias, const float* scale, const float* shift, int act, float* Y, long ldy,
                    long sy, const float* R1, long ldr1, long sr1, const float* R2, long ldr2, long sr2, void* stream);
/* Which block tile dispu_linear picks for (batch, M, N), as BM*1000 + BN (e.g. 128128): lets a profiler map a
 * launch to the kernel instantiation name rocprofv3 reports (linear_mfma_kernel<BM, BN, transb>). */
int dispu_linear_tile(int batch, int M, int N);
/* The same for a given K and transb (ABI 5): transposed-B products and K % 16 != 0 never take the DMA pipeline, which changes the
 * choice at 256 - 511 workgroups (64064 instead of 64128); dispu_linear_tile assumes the DMA pipeline. */
int dispu_linear_tile2(int batch, int M, int K, int N, int transb);
/* benchmarking aid (tools/gemm_bench.py): force the block tile of every later dispu_linear call; 0 restores the rule.  Not used by the product path. */
void dispu_debug_linear_tile(int code);
/* The launches a dispu_linear / dispu_linear_bn / dispu_linear_masked call with these arguments would make (debug / profiling
 * aid; the launchers run off the same decision).  Takes every argument of the three entries but the stream (scale / shift NULL for
 * dispu_linear, Mk NULL and mcols 0 without a mask).  Pointers are tested for NULL and alignment only and never dereferenced, and
 * no HIP call is made: it answers on a machine without a GPU.  Returns 0, or the error the call itself would return.
 * plan[0]: number of launches (0 for an empty product, 1, or 2 when the last N % 128 <= 32 columns go to the skinny kernel).
 * Launch i at plan[1 + 10 i ...]: kind (0 skinny kernel, 1 tiled kernel), first column, end column, then for the tiled kernel
 * BM, BN, BK, transb, edge (1: predicated loaders), EPI (0 plain, 1 BatchNorm fold, 4 residuals, 5 mask, 6 = 0 on the long-K
 * instantiation), 0; for the skinny kernel 0, 0, 0, transb, 0, 0, NG (k groups of 16 in registers: 2, 8, 16, 24).
 * Launches are listed in issue order.  Honours dispu_debug_linear_tile. */
#define DISPU_LINEAR_PLAN_INTS 21
int dispu_linear_plan(int batch, int M, int K, int N, const float* X, long ldx, long sx, const float* W, long ldw, long sw,
                      int transb, const float* bias, const float* scale, const float* shift, int act, const float* Y, long ldy,
                      long sy, const float* R1, long ldr1, long sr1, const float* R2, long ldr2, long sr2, const float* Mk,
                      long ldm, int mcols, int* plan);
/* K <= 4 inputs, N in {16, 24} outputs (feature_extraction layer0, ops.py:1449-1451). */
int dispu_linear_small_k(long rows, int K, int N, const float* X, long ldx, const float* W, const float* bias, int act,
                         float* Y, long ldy, void* stream);
/* N == 3 outputs (coordinate_regressor fc_layer2, ops.py:1101-1104); mode 1: Y = R + (sigmoid(.) - 0.5), the fine
 * branch's offset fused with `fine = coarse + offset` (ops.py:1106-1108, DisPU/generator.py:80-81). */
int dispu_linear_small_n(long rows, int K, int N, const float* X, long ldx, const float* W, const float* bias, int mode,
                         const float* R, long ldr, float* Y, long ldy, void* stream);
/* dense_conv + get_edge_feature fused (ops.py:1856-1877,1897-1915): F [npoints, C] (C in {24,48}), idx[npoints, ldi]
 * neighbour ids (columns ioff..ioff+15, cloud-local), three 1x1 convs with dense concat, max over the 16 neighbours.
 * Y[p, 0:72+C] = [max l2 | max l1 | max l0 | F_p]. */
int dispu_edge_dense_conv(int npoints, int n_per_cloud, int C, const float* F, long ldf, const int* idx, int ldi, int ioff,
                          const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                          const float* b2, float* Y, long ldy, void* stream);
/* One dense block of feature_extraction_GCN (ops.py:1437-1486) in one launch: knn_point_2(ksel, F, F) (tf_util.py:618-651; the
 * dispu_knn_feat_strided search) -> get_edge_feature over neighbours ioff .. ioff + 15 (ops.py:1856-1877) -> dense_conv (:1897-1915).
 * Bit-identical to dispu_knn_feat_strided followed by dispu_edge_dense_conv.  Clouds of up to 256 points (n_per_cloud even,
 * >= ksel = ioff + 16 <= 20; npoints a multiple of n_per_cloud); idx_out (nullable): the [npoints, ksel] neighbour table.
 * Wp (nullable) [72 + C + k_old, 48], bp [48]: the NEXT block's bottleneck conv (feature_extraction layer<d+1>_prep, ops.py:1455-1462)
 * in the same launch: P[p, 0:48] = relu([Y[p, 0:72+C] | Y[p, 72+C : 72+C+k_old]] . Wp + bp) -- Y's row continues to the right with the
 * k_old (a multiple of 24) older feature columns; bit-identical to dispu_linear on those rows (where the conv's operands do not fit in
 * the LDS the cloud leaves -- small clouds, many older columns -- it is a dispu_linear launch after the block).
 * xyz (nullable; C == 24, clouds of <= 680 points) [npoints, 3]: F is not read -- the block's input is feature_extraction's layer0
 * (ops.py:1449-1451) = xyz . Wl [3, 24] + bl, evaluated while the cloud is staged (bit-identical to dispu_linear_small_k) and also
 * written to Lout [npoints, 24] (row stride ldl). */
int dispu_stem_block(int npoints, int n_per_cloud, int C, const float* F, long ldf, int ksel, int ioff, const float* W0, const float* b0,
                     const float* W1, const float* b1, const float* W2, const float* b2, float* Y, long ldy, int* idx_out, const float* Wp,
                     const float* bp, int k_old, float* P, long ldp, const float* xyz, const float* Wl, const float* bl, float* Lout,
                     long ldl, void* stream);
/* Same contract as dispu_edge_dense_conv, VALU formulation (one lane per pair, weights through scalar loads).
 * Bit-identical results; kept as the A/B twin of the MFMA kernel for tests and profiling. */
int dispu_edge_dense_conv_valu(int npoints, int n_per_cloud, int C, const float* F, long ldf, const int* idx, int ldi,
                               int ioff, const float* W0, const float* b0, const float* W1, const float* b1,
                               const float* W2, const float* b2, float* Y, long ldy, void* stream);
/* duplicate_up conv1 tail (ops.py:1161-1191): continues the per-source-point chain H with the two grid-code channels of
 * each of the `up` copies, + bias, ReLU.  Output rows are copy-major: (cloud*up + r)*n + i. */
int dispu_dup_grid(int nclouds, int n, int co, int up, const float* H, long ldh, const float* Wg, const float* bias,
                   const float* grid, float* Y, long ldy, void* stream);
/* PointShuffle2 (ops.py:1012-1087) pieces; idx [rows, k] int32 cloud-local neighbour ids from dispu_knn_xyz. */
int dispu_ps_prep(long rows, int co, const float* xyz, const float* W0, const float* bias, float* G, long ldg, float* A,
                  long lda, void* stream);
int dispu_ps_gather_sub_relu(long rows, int n_per_cloud, int k, int c, const int* idx, const float* G, long ldg,
                             const float* A, long lda, float* X1, long ldx1, void* stream);
int dispu_ps_skip_max(long rows, int n_per_cloud, int k, int cf, const int* idx, const float* xyz, const float* feat,
                      long ldf, float* out, long ldo, void* stream);
int dispu_ps_weight_net(long rows, int n_per_cloud, int k, int t_n, const int* idx, const float* xyz, const float* Ww,
                        const float* bw, const float* scale, const float* shift, float* wv, void* stream);
int dispu_ps_point_matmul(long rows, int k, int c, int t_n, const float* X2, long ldx2, const float* wv, float* out,
                          long ldo, void* stream);
/* PointShuffle2 local cell fused (ops.py:1055-1067): gather_sub_relu -> conv1 (W1 [128,128], b1) -> weight_net ->
 * per-point feature x weight product, in one kernel; out [npoints, 2048].  Bit-identical to the chain
 * dispu_ps_gather_sub_relu / dispu_linear / dispu_ps_weight_net / dispu_ps_point_matmul; k == 16, c == 128. */
int dispu_ps_local(long npoints, int n_per_cloud, int k, int c, const int* idx, const float* xyz, const float* G, long ldg,
                   const float* A, const float* W1, const float* b1, const float* Ww, const float* bw, const float* scale,
                   const float* shift, float* out, void* stream);
/* dispu_ps_local (ops.py:1055-1067) with F' STORED AS bf16: out is bf16 [npoints, 2048], every element the fp32 value dispu_ps_local
 * writes rounded to nearest even -- the operand rounding of a bf16 after_conv product (ops.py:1078), done at the store, at half the
 * bytes.  Same arguments and checks otherwise (k == 16, c == 128, 16-byte aligned G / A / W1 / out). */
int dispu_ps_local_bf16(long npoints, int n_per_cloud, int k, int c, const int* idx, const float* xyz, const float* G, long ldg,
                        const float* A, const float* W1, const float* b1, const float* Ww, const float* bw, const float* scale,
                        const float* shift, void* out, void* stream);
/* PointNonLocalCell attention fused (ops.py:326-339): O[b,m,64] = softmax(scale * Q.K^T) . V per cloud, logits never
 * written to HBM.  d must be 64, nk % 32 == 0, rows 16-byte aligned (else hipErrorInvalidValue: use the 3-kernel path). */
int dispu_attention(int b, int m, int nk, int d, const float* Q, long ldq, const float* K, long ldk, const float* V,
                    long ldv, float scale, float* O, long ldo, void* stream);
/* The same cell including its output projection conv_back_project (ops.py:341-343: 64 -> n_out = 256 channels, bias,
 * ReLU) as the kernel's epilogue: Y[b*m, 256] = relu(softmax(scale Q K^T) V W + bias); the [b*m, 64] attention output is
 * never written.  W [64, 256] row-major, bias [256]. */
int dispu_attention_project(int b, int m, int nk, int d, const float* Q, long ldq, const float* K, long ldk, const float* V,
                            long ldv, float scale, const float* W, const float* bias, int n_out, float* Y, long ldy,
                            void* stream);
/* The cell's attention for the TRAINING step, without the [b, m, nk] probability tensor the reference keeps for its backward pass
 * (tf.matmul / tf.nn.softmax / tf.matmul of ops.py:326-339 and their TF1 gradients).  Forward: O as dispu_attention, plus
 * lse2[b*m] = log2 sum_k 2^(scale log2(e) Q.K) per query.  Backward: P is recomputed tile by tile from Q, K and lse2; writes
 * (overwrites) dQ [b*m, 64], dK / dV [b*nk, 64]; dvec [b*m] floats of scratch (receives rowsum(dO o O)).  Two launches, no float
 * atomics (run-to-run identical).  d == 64, m % 32 == 0, nk % 32 == 0, every row 16-byte aligned. */
int dispu_attention_fwd_lse(int b, int m, int nk, int d, const float* Q, long ldq, const float* K, long ldk, const float* V,
                            long ldv, float scale, float* O, long ldo, float* lse2, void* stream);
int dispu_attention_bwd(int b, int m, int nk, int d, const float* Q, long ldq, const float* K, long ldk, const float* V, long ldv,
                        float scale, const float* O, long ldo, const float* lse2, const float* dO, long lddo, float* dQ, long lddq,
                        float* dK, long lddk, float* dV, long lddv, float* dvec, void* stream);
/* S <- softmax(S * mul) per row of n columns (any n), in place (tf.nn.softmax of PointNonLocalCell, ops.py:338). */
int dispu_softmax_rows(long rows, int n, float mul, float* S, long lds, void* stream);

/* Fused head chains (one launch, activations stay in LDS): X [rows, K0] -> relu(. W1 + b1) [N1] -> relu(. W2 + b2) [N2]
 * -> relu(. W3 + b3) [N3] -> . W4 + b4 [3]; mode 1: out = R + sigmoid(.) - 0.5.  Y1 (optional) receives the first
 * layer's output.  Coarse head: upshuffle conv2 + coordinate_regressor (ops.py:1186-1192, 1089-1104), shape
 * (256,128,256,64); fine head: PointShuffle2 aggregation + coordinate_regressor is_off (ops.py:1079-1083, 1089-1108),
 * shape (256,256,256,64).  rows % 128 == 0.  Bit-identical to the dispu_linear / dispu_linear_small_n launches. */
int dispu_mlp_chain(long rows, int K0, int N1, int N2, int N3, const float* X, long ldx, const float* W1, const float* b1,
                    const float* W2, const float* b2, const float* W3, const float* b3, const float* W4, const float* b4,
                    float* Y1, long ldy1, int mode, const float* R, long ldr, float* out, long ldo, void* stream);
/* Round 4: the same chain with its input tile formed by the loader waves instead of a producer kernel.
 * _sum3: input = (X + X2) + X3, three [rows, K0] matrices with one row stride (PointShuffle2's relu(after_conv) + skip + non-local,
 *        ops.py:1069-1075: the two residual reads leave the after_conv GEMM's epilogue).
 * _dup:  input = duplicate_up's conv1 rows (ops.py:1152-1192) evaluated from the per-source-point product H [nclouds*n, K0]:
 *        row (cloud*up + r)*n + i = relu(fmaf(grid[r][1], Wg[1], fmaf(grid[r][0], Wg[0], H[cloud*n + i])) + bg) -- dispu_dup_grid's
 *        arithmetic without its [nclouds*up*n, K0] output.  Both are bit-identical to producer + dispu_mlp_chain. */
int dispu_mlp_chain_sum3(long rows, int K0, int N1, int N2, int N3, const float* X, const float* X2, const float* X3, long ldx,
                         const float* W1, const float* b1, const float* W2, const float* b2, const float* W3, const float* b3,
                         const float* W4, const float* b4, float* Y1, long ldy1, int mode, const float* R, long ldr, float* out, long ldo,
                         void* stream);
int dispu_mlp_chain_dup(int nclouds, int n, int up, int K0, int N1, int N2, int N3, const float* H, long ldh, const float* Wg,
                        const float* bg, const float* grid, const float* W1, const float* b1, const float* W2, const float* b2,
                        const float* W3, const float* b3, const float* W4, const float* b4, float* Y1, long ldy1, int mode, const float* R,
                        long ldr, float* out, long ldo, void* stream);

/* ---- glue kernels of the PointNet++ / EdgeConv / loss compositions --------------------------------------
 * (Common/pointnet_util.py, gcn_lib/tf_vertex.py, Common/loss_utils.py: chains of generic TF ops in the reference) */
/* grouped[r,s,:] -= center[r,:]  ("translation normalization", pointnet_util.py:43; loss_utils.py:281). */
int dispu_group_center(long rows, int ns, int c, float* grouped, const float* center, void* stream);
/* pointnet_sa_module's hot loop fused (pointnet_util.py:91-149 with pooling 'max', mlp2 None, use_xyz, inference BatchNorm):
 * out[b,m,cout[nl-1]] = max_s mlp([xyz[idx[b,m,s]] - new_xyz[b,m] | points[idx[b,m,s]]]) -- group_point, the translation
 * normalisation, nl <= 3 conv2d layers (bias, optional BatchNorm fold scale/shift, ReLU) and the max over nsample in one
 * launch; the [b,m,ns,C] tensors never reach HBM.  ns in {32, 64}; W[l] [cin_l, cout_l] row-major, cin_0 = 3 + c (c = 0:
 * points may be NULL), cin_l = cout[l-1]; scale / shift may be NULL (no BatchNorm) or hold NULL entries.  Bit-identical to
 * dispu_group_point -> dispu_group_center -> dispu_linear_bn x nl -> dispu_pool_nsample(max). */
int dispu_sa_fused(int b, int n, int m, int ns, int c, const float* xyz, const float* new_xyz, const float* points, const int* idx,
                   int nl, const float* const* W, const float* const* bias, const float* const* scale, const float* const* shift,
                   const int* cout, float* out, void* stream);
/* EdgeConv fused (gcn_lib/tf_vertex.py:81-101 over tf_util.get_edge_feature, Common/tf_util.py:654-686):
 * out[i,:] = max_{s<k} mlp([F[i] | F[idx[i,s]] - F[i]]), nl <= 3 conv2d layers (bias, optional BatchNorm fold, ReLU; the last layer's
 * ReLU only when act_last), k in {16, 32, 64}; feat [b*n, c] (row stride ldf), idx [b*n, >= k] cloud-relative (row stride ldi).
 * Neither the [b,n,k,2c] edge tensor nor a [b,n,k,C] layer output reaches HBM.  Bit-identical to dispu_edge_feature ->
 * dispu_linear_bn x nl -> dispu_pool_nsample(max). */
int dispu_edge_conv_fused(int b, int n, int k, int c, const float* feat, long ldf, const int* idx, int ldi, int nl,
                          const float* const* W, const float* const* bias, const float* const* scale, const float* const* shift,
                          const int* cout, int act_last, float* out, void* stream);
/* pooling over nsample of X[rows,ns,c] (pointnet_util.py:121-140): mode 0 max, 1 avg, 2 "min" (= max(-x), as the
 * reference computes it), 3 weighted_avg (needs gxyz[rows,ns,3]), 4 max_and_avg -> [max|avg] (2c outputs),
 * 5 sum (GIN aggregation, gcn_lib/tf_vertex.py:248). */
int dispu_pool_nsample(long rows, int ns, int c, int mode, const float* X, const float* gxyz, float* out, void* stream);
/* tf.nn.l2_normalize(x, axis=-1) of GraphSAGE (gcn_lib/tf_vertex.py:133-134): out[r,:] = X[r,:] / sqrt(max(sum_c X[r,c]^2, 1e-12)). */
int dispu_l2_normalize_rows(long rows, int c, const float* X, float* out, void* stream);
/* out = x * alpha + y elementwise (GIN: inputs * (1 + epsilon) + aggregated, gcn_lib/tf_vertex.py:205). */
int dispu_scale_add(long n, const float* x, float alpha, const float* y, float* out, void* stream);
/* pointnet_fp_module inverse-distance weights (pointnet_util.py:204-208): dist[rows,3] -> weight[rows,3]. */
int dispu_idw_weights(long rows, const float* dist, float* weight, void* stream);
/* tf_util.get_edge_feature (Common/tf_util.py:654-686): out[(i,s), 0:2c] = [F_i | F_j - F_i]. */
int dispu_edge_feature(long rows, int n_per_cloud, int k, int c, const float* F, long ldf, const int* idx, int ldi, int ioff,
                       float* out, long ldo, void* stream);
/* per-row mean and max of x[b,n] (Chamfer / Hausdorff reductions, loss_utils.py:59-63,78-83). */
int dispu_row_mean_max(int b, int n, const float* x, float* mean, float* mx, void* stream);
/* get_repulsion_loss core (loss_utils.py:280-296): out[i] = sum of max(0, h - d) over the 2nd..5th smallest
 * neighbour distances of point i among idx[i, 0:ns]. */
int dispu_repulsion(long rows, int n_per_cloud, int ns, int use_l1, float h, const float* pred, const int* idx, float* out,
                    void* stream);

/* ---- training step (DisPU/model.py:68-87 loss, :158-178 AdamOptimizer.minimize) ---------------------------------
 * The reference has no native code here: TF1 autodiff derives every gradient from the forward graph.  These entry
 * points are those gradients written out; each cites the forward op it differentiates.  Convention: for a layer
 * Y = act(X.W + b):  dZ = dY * act'(Y) (dispu_act_bias_grad, which also yields db = colsum dZ),
 * dW = X^T.dZ (dispu_linear_tn),  dX = dZ.W^T (dispu_linear with transb = 1, R1 = dX to accumulate). */
/* Mixed-precision variants for the training step (BASELINE configs[4] names bf16; the reference itself is fp32-only, so this
 * is an opt-in extension, Trainer(dtype="bf16")): same contracts as dispu_linear / dispu_linear_tn, fp32 tensors in memory,
 * operands rounded to bf16 (RNE) on the way into LDS, v_mfma_f32_32x32x16_bf16 products, fp32 accumulation and epilogue.
 * dispu_linear_tn_bf16's dbias (optional, batch == 1) is an fp32 column sum of the UN-rounded Z, taken inside the kernel. */
int dispu_linear_bf16(int batch, int M, int K, int N, const float* X, long ldx, long sx, const float* W, long ldw, long sw,
                      int transb, const float* bias, int act, float* Y, long ldy, long sy, const float* R1, long ldr1, long sr1,
                      const float* R2, long ldr2, long sr2, void* stream);
long dispu_linear_tn_bf16_scratch_floats(int batch, int M, int K, int N);
int dispu_linear_tn_bf16(int batch, int M, int K, int N, const float* X, long ldx, long sx, const float* Z, long ldz, long sz,
                         float* out, long ldo, long so, int accumulate, float* dbias, float* scratch, long scratch_floats,
                         void* stream);
/* EXPLORATORY, opt-in (Generator.split_bf16 / bench.py --split-bf16; never the default): fp32-accurate products on the bf16
 * matrix pipe.  Operands are split into three bf16 terms each (24 mantissa bits), the six partial products of order <= 2 are
 * exact bf16 MFMAs accumulated in fp32.  Not the ascending-k fmaf chain of dispu_linear: offered only for the generator's
 * tolerance-checked refinement branch.  dispu_bf16x3_split_weights writes W's planes once ([3][N][K] bf16, 6 K N bytes);
 * dispu_linear_bf16x3: Y = R2 + R1 + act(X . W + bias), M % 128 == N % 128 == K % 32 == 0. */
int dispu_bf16x3_split_weights(int K, int N, const float* W, long ldw, void* planes, void* stream);
int dispu_linear_bf16x3(int M, int K, int N, const float* X, long ldx, const void* planes, const float* bias, int act, float* Y,
                        long ldy, const float* R1, long ldr1, const float* R2, long ldr2, void* stream);
/* benchmarking aid (tools/debug/x3_lab.py, x3_step_ab.py, tests): 1 = round 4's wave-specialised kernel (default), 0 = round 6's streaming kernel
 * for the N % 256 == 0 shapes; same planes, bit-identical results.  Not used by the product path. */
void dispu_debug_x3_kernel(int which);
/* floats of scratch dispu_linear_tn needs for (batch, M, K, N). */
long dispu_linear_tn_scratch_floats(int batch, int M, int K, int N);
/* out[z][k][n] (+)= sum_m X[z][m][k] * Z[z][m][n]   (conv2d_backprop_filter of a 1x1 conv; the TN products of the
 * attention backward, ops.py:326-339);  dbias[n] += sum_m Z[m][n] when non-NULL (bias_add_grad rides along as one
 * extra output row).  Deterministic: M-splits are summed in a fixed order from `scratch`. */
int dispu_linear_tn(int batch, int M, int K, int N, const float* X, long ldx, long sx, const float* Z, long ldz, long sz,
                    float* out, long ldo, long so, int accumulate, float* dbias, float* scratch, long scratch_floats,
                    void* stream);
/* What a dispu_linear_tn / dispu_linear_tn_bf16(s) / dispu_linear_tn_bf16_stream call with these arguments would launch (debug / test aid
 * like dispu_linear_plan; each launcher switches over the same host decision).  Every argument of the entry but the stream; pointers are
 * tested for NULL and alignment only and never dereferenced, no HIP call is made.  Returns 0, or the error the entry itself would return
 * (the plan is then all zero).  The three entries refuse a NULL `out`, and NULL X / Z when M > 0.
 * dispu_linear_tn_plan, plan[0..11]: kind (0 nothing to launch, 1 narrow kernel, 2 tiled kernel, 3 M == 0: `out` is cleared unless
 *   accumulating), TK, TNN, edge (tiled: block tile 64 TK x 64 TNN, predicated loaders), splits (narrow: chunks), rows per split, direct
 *   (the product kernel writes `out` itself: one split, no accumulate, no dbias; scratch may be NULL), reduce (0 none, 1 scalar, 2 float4
 *   kernel), the reduction's grid, capped (1: that grid is at its limit and loops), then for the narrow kernel waves per block and grid.y.
 * dispu_linear_tn_bf16_plan (arguments of dispu_linear_tn_bf16s), plan[0..5]: kind (0, 2 product, 3 M == 0: `out` and dbias are cleared
 *   unless accumulating), block tile (128032 / 64064 / 128128), splits, rows per split, reduce (1: partial tiles + reduction; 0: one
 *   workgroup per tile writes `out`, scratch unused), rows of a partial (K, or K + 1 with dbias).
 * dispu_linear_tn_bf16_stream_plan, plan[0..3]: BN (256 / 128), storage (0 / 3), splits, rows per split; always partials + reduction. */
#define DISPU_LINEAR_TN_PLAN_INTS 12
int dispu_linear_tn_plan(int batch, int M, int K, int N, const float* X, long ldx, long sx, const float* Z, long ldz, long sz,
                         const float* out, long ldo, long so, int accumulate, const float* dbias, const float* scratch,
                         long scratch_floats, int* plan);
#define DISPU_LINEAR_TN_BF16_PLAN_INTS 6
int dispu_linear_tn_bf16_plan(int batch, int M, int K, int N, const void* X, long ldx, long sx, const void* Z, long ldz, long sz,
                              const float* out, long ldo, long so, int accumulate, const float* dbias, const float* scratch,
                              long scratch_floats, int storage, int* plan);
#define DISPU_LINEAR_TN_BF16_STREAM_PLAN_INTS 4
int dispu_linear_tn_bf16_stream_plan(int M, int K, int N, const void* X, long ldx, const void* Z, long ldz, int storage, const float* out,
                                     long ldo, int accumulate, const float* dbias, const float* scratch, long scratch_floats, int* plan);
/* Deferred split reductions (ABI 5; csrc/train_gemm.hip).  The training step has ~20 weight-gradient products, each followed by its own
 * 4 - 25 us reduction launch that only Adam waits for.  dispu_tn_defer(&desc) arms a ONE-SHOT, per-thread sink: the next dispu_linear_tn /
 * dispu_linear_tn_bf16(s) / dispu_linear_tn_bf16_stream call on this thread (batch == 1) launches its product only and fills `desc` with the
 * reduction it left undone (desc.splits == 0: it left none); its `scratch` must then stay untouched until dispu_tn_reduce_grouped has run
 * those descriptors -- any number of them in ONE launch, `table_device` being a device copy of `table_host` (count entries), on a stream
 * ordered after the products.  Same association as the products' own reductions: bit-identical results.  Descriptors of one call must not
 * alias each other's `out` rows or `dbias`. */
typedef struct dispu_tn_reduce_desc {
    const float* part; float* out; float* dbias;
    long ldo, stride;
    int K, N, splits, rows_p;
    int accumulate, bias_accumulate, assoc, reserved;
} dispu_tn_reduce_desc;
int dispu_tn_defer(dispu_tn_reduce_desc* desc);
int dispu_tn_reduce_grouped(int count, const dispu_tn_reduce_desc* table_host, const dispu_tn_reduce_desc* table_device, void* stream);
long dispu_act_bias_grad_scratch_floats(long rows, int n);
/* dZ = dY * (act ? Y > 0 : 1) (relu_grad; dZ may be NULL, or dY itself with lddz == lddy: any other stride under the same pointer is
 * refused), dbias (+)= column sums of dZ (bias_add_grad;
 * dbias may be NULL).  tf_util.py:100-115,170-185. */
int dispu_act_bias_grad(long rows, int n, const float* dY, long lddy, const float* Y, long ldy, int act, float* dZ, long lddz,
                        float* dbias, int accumulate, float* scratch, long scratch_floats, void* stream);
/* tf.reduce_max over the neighbour axis, strided (ops.py:1915, :1049): out[i, c] = max_s X[(i*ns + s), c]. */
int dispu_max_k(long rows, int ns, int c, const float* X, long ldx, float* out, long ldo, void* stream);
/* its gradient (math_grad._MinOrMaxGrad: shared evenly by tied maxima). */
int dispu_max_k_grad(long rows, int ns, int c, const float* X, long ldx, const float* Y, long ldy, const float* dY, long lddy,
                     float* dX, long lddx, int accumulate, void* stream);
/* the same, overwriting, plus zeros into the `tail` columns behind the c pooled ones (the part of a dense block's gradient
 * buffer that only accumulates afterwards: saves a separate fill). */
int dispu_max_k_grad_tail(long rows, int ns, int c, int tail, const float* X, long ldx, const float* Y, long ldy, const float* dY,
                          long lddy, float* dX, long lddx, void* stream);
/* gradient of get_edge_feature (ops.py:1856-1877): dF accumulates (atomics); dE [(rows*k), 2c]. */
int dispu_edge_feature_grad(long rows, int n_per_cloud, int k, int c, const float* dE, long lde, const int* idx, int ldi,
                            int ioff, float* dF, long lddf, void* stream);
/* gradient of duplicate_up's tile (ops.py:1152-1199): dH[cloud*n + i] = sum_r dZ[(cloud*up + r)*n + i]. */
int dispu_dup_sum_grad(int nclouds, int n, int co, int up, const float* dZ, long lddz, float* dH, long lddh, void* stream);
/* PointShuffle2 grouping, materialised (ops.py:1030-1037): gf[(i,s), 0:6+cf] = [xyz_j - xyz_i | xyz_j | feat_j]. */
int dispu_ps_group(long rows, int n_per_cloud, int k, int cf, const int* idx, const float* xyz, const float* feat, long ldf,
                   float* gf, long ldg, void* stream);
/* its gradient: dxyz [rows,3] and dfeat [rows, cf] accumulate (atomics). */
int dispu_ps_group_grad(long rows, int n_per_cloud, int k, int cf, const int* idx, const float* dgf, long ldg, float* dxyz,
                        float* dfeat, long lddf, void* stream);
/* gradient of dispu_ps_point_matmul (tf.matmul, ops.py:1063-1064); k == t_n == 16, c == 128. */
int dispu_ps_point_matmul_grad(long rows, int k, int c, int t_n, const float* X2, long ldx2, const float* wv, const float* dout,
                               long ldo, float* dX2, long lddx2, float* dwv, void* stream);
/* gradient of dispu_softmax_rows: dP <- mul * P * (dP - rowsum(dP * P)), in place. */
int dispu_softmax_rows_grad(long rows, int n, float mul, const float* P, long ldp, float* dP, long lddp, void* stream);
/* scratch that serves both entries below: the gradient's three double partial sums per block and channel (the forward needs, and
 * checks for, two of them). */
long dispu_bn_scratch_bytes(long rows, int c);
/* contrib.layers.batch_norm in training mode (tf_util.py:512-531): batch statistics over the rows, eps, optional
 * ReLU; stats[3c] = mean | biased var | 1/sqrt(var+eps); moving statistics updated in place with `decay`. */
int dispu_bn_train(long rows, int c, const float* X, long ldx, const float* gamma, const float* beta, float eps, float decay,
                   int act, float* Y, long ldy, float* stats, float* moving_mean, float* moving_var, void* scratch,
                   long scratch_bytes, void* stream);
/* its gradient: dX written, dgamma / dbeta accumulate, sums[2c] receives (sum dz | sum dz*xhat); xhat about the true mean: the
 * offset of the float32 mean in `stats` is measured (sum xhat) and taken out. */
int dispu_bn_train_grad(long rows, int c, const float* X, long ldx, const float* Y, long ldy, const float* dY, long lddy,
                        const float* stats, const float* gamma, int act, float* dX, long lddx, float* dgamma, float* dbeta,
                        float* sums, void* scratch, long scratch_bytes, void* stream);
/* out = base + sigmoid(z) - 0.5 (coordinate_regressor is_off, ops.py:1106-1108; generator.py:80-81) and its gradient
 * (dz written; dbase accumulates when non-NULL). */
int dispu_sigmoid_offset(long total, const float* z, const float* base, float* out, void* stream);
int dispu_sigmoid_offset_grad(long total, const float* z, const float* dout, float* dz, float* dbase, void* stream);
/* gradient of get_repulsion_loss (loss_utils.py:280-296) w.r.t. pred, times `scale`; dpred accumulates (atomics). */
int dispu_repulsion_grad(long rows, int n_per_cloud, int ns, float h, float scale, const float* pred, const int* idx,
                         float* dpred, void* stream);
/* out = (a + b) + c  (tf.add x2, ops.py:1072-1075). */
int dispu_add3(long total, const float* a, const float* b, const float* c, float* out, void* stream);
/* Second half of a split-K product for FEW rows and a LONG contraction (the training forward's after_conv at 8 - 16 patches:
 * [8192 x 2048] x [2048 x 256] gives 64 tiles of 128 x 256 -- a quarter of the chip -- or 512 L2-bound 64 x 64 tiles): the caller runs
 * dispu_linear with batch = nparts over K-chunks (sx = K / nparts, sw = (K / nparts) * ldw, no bias / activation, partials [nparts][rows][n]
 * with stride part_stride) and this adds them in ascending chunk order, then bias, then the activation:
 * Y = act(((P_0 + P_1) + ...) + bias).  A reassociation of the ascending-k chain: only used where the result is tolerance-checked. */
int dispu_linear_splitk_finish(long rows, int n, int nparts, const float* part, long part_stride, const float* bias, int act, float* Y,
                               long ldy, void* stream);
/* out[b, j] = val[b] * mul (the constant rows d loss / d dist of chamfer's means, loss_utils.py:59-63). */
int dispu_fill_rows(int b, int n, const float* val, float mul, float* out, void* stream);
/* tf.train.AdamOptimizer update on flat buffers (model.py:178); g is scaled by gscale first (1/world after the
 * gradient all-reduce). */
int dispu_adam(long total, float* p, const float* g, float* m, float* v, float lr_t, float beta1, float beta2, float eps,
               float gscale, void* stream);

/* ---- training step, round 3: fused forward + backward of the PointShuffle2 local cell / skip branch without the [B*M*16, 134]
 * pair tensors (csrc/train_fused.hip), ReLU gradients folded into the GEMM epilogues, head chains with stashed activations ---- */
/* dispu_linear followed by a ReLU-gradient mask: Y[m][n] = 0 where Mk[m][n] <= 0, for the columns n < mcols of this product
 * (dX = dZ.W^T (+ R1) of a layer whose INPUT was the ReLU output Mk: relu_grad of the layer below, tf_util.py:100-115). */
int dispu_linear_masked(int batch, int M, int K, int N, const float* X, long ldx, long sx, const float* W, long ldw, long sw,
                        int transb, const float* bias, int act, float* Y, long ldy, long sy, const float* R1, long ldr1, long sr1,
                        const float* Mk, long ldm, int mcols, void* stream);
int dispu_linear_bf16_masked(int batch, int M, int K, int N, const float* X, long ldx, long sx, const float* W, long ldw, long sw,
                             int transb, const float* bias, int act, float* Y, long ldy, long sy, const float* R1, long ldr1, long sr1,
                             const float* Mk, long ldm, int mcols, void* stream);
/* The block tile dispu_linear_bf16 / _bf16s / _bf16_masked (splits = 1) and the dispu_linear_tn_bf16* products launch for an
 * M x N output per batch entry, as BM*1000 + BN: 128032 (N <= 32), 64064 (fewer than 512 tiles of 128 x 128 over splits and batch)
 * or 128128; 0 for an empty product.  Debug / profiling aid like dispu_linear_plan: no HIP call. */
int dispu_linear_bf16_plan(int batch, int M, int N, int splits);
/* Streaming bf16-product GEMM for the step's largest dense products (Trainer(dtype="bf16"); csrc/linear_bf16_stream.hip): operands by
 * DMA into LDS, X fp32 rounded to bf16 (nearest even) in front of the matrix pipe, B supplied as Bt [N][K] bf16 (k contiguous) by
 * dispu_bf16_pack (transpose = 1 of W [K][N] for Y = X.W; transpose = 0 of W [N][K] for dX = dZ.W^T).  Same products as
 * dispu_linear_bf16; x_bf16 / y_bf16: X / Y stored as bf16; splits > 1: fp32 partial products of `splits` equal k ranges to
 * Y + s * y_split, no bias / activation (dispu_linear_splitk_finish adds them in order).  M % 128 == 0, K % (32 splits) == 0,
 * N % 128 == 0, 16-byte aligned rows -- anything else returns hipErrorInvalidValue (the caller keeps dispu_linear_bf16). */
int dispu_bf16_pack(int rows, int cols, const float* W, long ldw, int transpose, void* out, void* stream);
/* dW = X^T . Z on the streaming kernel: X [M][K], Z [M][N] both fp32 (storage = 0) or both bf16 (storage = 3); out [K][N] (+)=, dbias [N]
 * (+)= column sums of Z (optional).  scratch: dispu_linear_tn_bf16_stream_scratch_floats(M, K, N) floats; 0 = shape outside the kernel
 * (K % 128, N % 128, rows divisible into 32-row slabs per split) -- dispu_linear_tn_bf16_stream then returns hipErrorInvalidValue. */
long dispu_linear_tn_bf16_stream_scratch_floats(int M, int K, int N);
int dispu_linear_tn_bf16_stream(int M, int K, int N, const void* X, long ldx, const void* Z, long ldz, int storage, float* out, long ldo,
                                int accumulate, float* dbias, float* scratch, long scratch_floats, void* stream);
int dispu_linear_bf16_stream(int M, int K, int N, const void* X, long ldx, int x_bf16, const void* Bt, long ldb, const float* bias, int act,
                             void* Y, long ldy, int y_bf16, int splits, long y_split, void* stream);
/* dispu_mlp_chain that also writes the second / third layer's outputs (Y2 [rows,N2], Y3 [rows,N3]) and the head's pre-activation
 * output Z [rows,3]: the training forward of the two head chains in one launch each (any of Y1, Y2, Y3, Z may be NULL). */
int dispu_mlp_chain_stash(long rows, int K0, int N1, int N2, int N3, const float* X, long ldx, const float* W1, const float* b1,
                          const float* W2, const float* b2, const float* W3, const float* b3, const float* W4, const float* b4,
                          float* Y1, long ldy1, float* Y2, long ldy2, float* Y3, long ldy3, float* Z, long ldz, int mode,
                          const float* R, long ldr, float* out, long ldo, void* stream);
/* Backward of dispu_mlp_chain(_stash) in one launch (csrc/mlp_chain_bwd.hip; replaces the four dX products TF autodiff generates for
 * upshuffle conv2 + coordinate_regressor / aggregation + fine regressor, ops.py:1186-1192, 1089-1108, 1079-1083):
 *   dY3 = (dZ.W4^T)*[Y3>0] -> D3 [rows,64];  dY2 = (dY3.W3^T)*[Y2>0] -> D2 [rows,N2];  dY1 = (dY2.W2^T + R + R2)*[Y1>0] -> D1 [rows,N1]
 *   (R, R2 optional gradients that reached Y1 through other consumers, N1 = 128 only; D1 may alias either);  dX = dY1.W1^T -> Da / Db / Dc [rows,K0] through the masks Ma / Mb / Mc (Ma NULL: unmasked; Db, Dc
 *   optional).  Wt3 / Wt2 / Wt1 are the TRANSPOSED forward weights, row-major [64,N2] / [N2,N1] / [N1,K0]; W4 the forward [64,3].
 * rows % 64 == 0; (K0,N1,N2) in {(256,128,256), (256,256,256)}; 16-byte aligned pointers.  The weight gradients are separate
 * dispu_linear_tn products over the stashed activations and D3 / D2 / D1. */
int dispu_mlp_chain_grad(long rows, int K0, int N1, int N2, const float* dZ, long lddz, const float* W4, const float* Wt3,
                         const float* Wt2, const float* Wt1, const float* Y3, long ldy3, const float* Y2, long ldy2,
                         const float* Y1, long ldy1, const float* R, long ldr, const float* R2, long ldr2, float* D3, long ldd3,
                         float* D2, long ldd2, float* D1, long ldd1, const float* Ma, const float* Mb, const float* Mc, long ldm, float* Da, float* Db,
                         float* Dc, long ldd0, void* stream);
/* Backward of dispu_ps_local in one recomputing launch (csrc/ps_local_bwd.hip; what TF autodiff derives from Common/ops.py:1055-1067):
 * given dF [npoints, 2048] = d loss / d F', per 8-point group h0 = relu(G[j] - A[i]) and h1 = relu(h0.W1 + b1) are rebuilt on chip with the
 * forward's arithmetic and   dwv[(i,s),t] = sum_c dF[i,c,t] h1[(i,s),c]   (-> dispu_ps_wnet_grad),
 * dz1 = (sum_t dF[i,c,t] wv[(i,s),t]) [h1 > 0]  [npoints*16, 128]  (-> the dW1 = h0^T.dz1 product),   dz0 = (dz1.W1^T) [h0 > 0],
 * dG[j] += dz0[(i,s)] (float atomics: dG must be ZERO on entry),   dAneg[i] = -sum_s dz0[(i,s)].
 * W1t = W1^T row-major [128, 128]; scale / shift = the weight net's folded BatchNorm of this step; k = 16, c = 128, t = 16. */
int dispu_ps_local_grad(long npoints, int n_per_cloud, const int* idx, const float* xyz, const float* Gm, long ldg, const float* Am,
                        const float* W1, const float* b1, const float* W1t, const float* Ww, const float* bw, const float* scale,
                        const float* shift, const float* dF, float* dz1, float* dwv, float* dG, float* dAneg, void* stream);
/* o_i = dY * (Y_i > 0), i = 1..3: the gradients of sum = relu(after_conv) + relu(skip) + relu(non-local) (ops.py:1072-1075). */
int dispu_mask3(long rows, int n, const float* dY, long lddy, const float* Y1, long ld1, const float* Y2, long ld2, const float* Y3,
                long ld3, float* o1, float* o2, float* o3, long ldo, void* stream);
/* weight_net_hidden in training mode (ops.py:181-191: conv 3 -> 16 of xyz_j - xyz_i, contrib batch_norm on BATCH statistics, ReLU)
 * without storing its [rows*16, 16] input: stats[48] = mean | biased var | 1/sqrt(var+eps); scale/shift[16] = the folded BatchNorm
 * dispu_ps_local / dispu_ps_weight_net apply; moving statistics updated in place (decay).  scratch: dispu_ps_wnet_scratch_bytes. */
long dispu_ps_wnet_scratch_bytes(long rows);
int dispu_ps_wnet_bn_stats(long rows, int n_per_cloud, int k, int t_n, const int* idx, const float* xyz, const float* Ww, const float* bw,
                           const float* gamma, const float* beta, float eps, float decay, float* stats, float* scale, float* shift,
                           float* moving_mean, float* moving_var, void* scratch, long scratch_bytes, void* stream);
/* its gradient from dwv [rows*16, 16] (gradient w.r.t. the ReLU output): dWw [3,16], dbw, dgamma, dbeta accumulate; dxyz [rows,3]
 * accumulates (atomics) the gradient w.r.t. both points of every pair; sums[32] receives (sum u | sum u*xhat). */
int dispu_ps_wnet_grad(long rows, int n_per_cloud, int k, int t_n, const int* idx, const float* xyz, const float* Ww, const float* bw,
                       const float* stats, const float* scale, const float* shift, const float* gamma, const float* dwv, float* dWw,
                       float* dbw, float* dgamma, float* dbeta, float* dxyz, float* sums, void* scratch, long scratch_bytes, void* stream);
/* the k-NN graph idx [b, n, k] (cloud-local ids) inverted per cloud: off [b, n+1], inv [b, n*k] = the pair ids i*k + s with
 * idx[i,s] == j in off[j] .. off[j+1], ascending.  n <= 4096. */
int dispu_knn_invert(int b, int n, int k, const int* idx, int* off, int* inv, void* stream);
/* conv0 per source point (h0 = relu(G[j] - A[i]), dispu_ps_prep) backward from dh0 [rows*k, 128], the gradient w.r.t. h0:
 * dz0 = dh0 * (G[j] - A[i] > 0) (the ReLU decision re-derived from G / A; Gm == Am == NULL: dh0 is taken as already masked), then
 * dG[p] = sum of dz0 over the in-edges of p (a deterministic gather through the inverted graph), dAneg[p] = -sum_s dz0[(p,s)]. */
int dispu_ps_conv0_gather_grad(long rows, int n_per_cloud, int k, int c, const int* idx, const int* off, const int* inv, const float* dh0,
                               long ldz, const float* Gm, long ldgm, const float* Am, long ldam, float* dG, long ldg, float* dAneg, long lda,
                               void* stream);
/* the xyz side of dispu_ps_prep backward: dxyz += dG.(Wc+Wr)^T + dAneg.Wc^T (atomics); dW0[0:3] += xyz^T (dG + dAneg),
 * dW0[3:6] += xyz^T dG (atomics).  W0 [134, 128] (rows 0:3 = Wc, 3:6 = Wr). */
int dispu_ps_prep_grad(long rows, int co, const float* xyz, const float* W0, const float* dG, long ldg, const float* dAneg, long lda,
                       float* dxyz, float* dW0, void* stream);
/* gradient of dispu_ps_skip_max (max over the 16 neighbours of [xyz_j - xyz_i | xyz_j | feat_j], ops.py:1049) without the grouped
 * tensor: shared evenly by the entries equal to the maximum, accumulated (atomics) into dxyz [rows,3] and dfeat [rows, cf].
 * feat_is_relu != 0: feat is a ReLU output whose relu_grad the caller applies to dfeat afterwards; shares that would land on its
 * zeros (a maximum of 0 = a 16-way tie of ReLU zeros) are then not sent at all -- same dfeat after the mask, 10x fewer atomics. */
int dispu_ps_skip_max_grad(long rows, int n_per_cloud, int k, int cf, const int* idx, const float* xyz, const float* feat, long ldf,
                           const float* gmax, long ldm, const float* dgmax, long ldd, float* dxyz, float* dfeat, long lddf,
                           int feat_is_relu, void* stream);
/* Backward of dispu_edge_dense_conv in one launch (+ a fixed-order reduction of the per-workgroup weight-gradient partials): the
 * forward values are recomputed on chip from F / idx / the weights (bit-identical to the forward kernel's), nothing of the edge
 * tensor is stored.  dOut [npoints, 72 + C] = gradient of Y; dF [npoints, C] accumulates (atomics); dW* / db* accumulate.
 * scratch: dispu_edge_dense_conv_grad_scratch_floats(npoints, C) floats. */
long dispu_edge_dense_conv_grad_scratch_floats(int npoints, int C);
int dispu_edge_dense_conv_grad(int npoints, int n_per_cloud, int C, const float* F, long ldf, const int* idx, int ldi, int ioff,
                               const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                               const float* dOut, long lddo, float* dF, long lddf, float* dW0, float* db0, float* dW1, float* db1,
                               float* dW2, float* db2, float* scratch, long scratch_floats, void* stream);
/* the same in two halves (a caller may queue the second on another stream, ordered after the first by an event, to keep the weight
 * gradients off its critical path): _partials leaves dW* / db* as per-workgroup partial sums in `scratch`, _reduce adds them (fixed
 * order) to dW* / db*. */
int dispu_edge_dense_conv_grad_partials(int npoints, int n_per_cloud, int C, const float* F, long ldf, const int* idx, int ldi, int ioff,
                                        const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                                        const float* b2, const float* dOut, long lddo, float* dF, long lddf, float* scratch,
                                        long scratch_floats, void* stream);
int dispu_edge_dense_conv_grad_reduce(int npoints, int C, const float* scratch, long scratch_floats, float* dW0, float* db0, float* dW1,
                                      float* db1, float* dW2, float* db2, void* stream);
/* one Chamfer term of pu_loss from dispu_nn_distance's outputs (loss_utils.py:45-64; gradient tf_nndistance.py:31-37): value[0] =
 * mean_b[(mean d_gt + mean d_pred) / radius_b]; dpred [b, n_pred, 3] = d(coef * CD)/d pred (zero-filled, then accumulated). */
int dispu_chamfer_loss_grad(int b, int n_gt, const float* gt, int n_pred, const float* pred, const float* d_gt, const int* i_gt,
                            const float* d_pred, const int* i_pred, const float* radius, float coef, float* value, float* dpred,
                            void* stream);
/* out[5] = 1000 CD_coarse | 1000 CD_fine | repulsion_w * mean(rep) / 4 | pu_loss (model.py:87) | weight_fine; cd[2] = the two
 * values of dispu_chamfer_loss_grad, rep [nrep] = dispu_repulsion's per-point sums (NULL: no repulsion term). */
int dispu_pu_loss_finalize(const float* cd, const float* rep, long nrep, float wf, float rep_w, float* out, void* stream);
/* the train loop's five per-step meters (model.py:215-222) in one launch:
 *   row[5] = pu_loss | 1000 CD_coarse | 100 HD_coarse | 1000 CD_fine | 100 HD_fine
 * loss_out = dispu_pu_loss_finalize's out (its entries 3, 0, 1 are copied); d_gt_* [b, n_gt] / d_pred_* [b, n_pred] = the distances
 * dispu_nn_distance(gt, pred) left for the coarse (_c) and the fine (_f) cloud; radius [b].  Per term, hausdorff_loss
 * (loss_utils.py:67-84): 100.0f * max_b[(1.0f * max_j d_gt[b,j] + max_j d_pred[b,j]) / radius[b]] with an IEEE fp32 division.  `row` is
 * any 5 floats of a caller-owned table; nothing else is written.  b <= 0, n_* <= 0 or a NULL pointer: hipErrorInvalidValue, no
 * launch. */
int dispu_step_meters(int b, int n_gt, int n_pred, const float* d_gt_c, const float* d_pred_c, const float* d_gt_f,
                      const float* d_pred_f, const float* radius, const float* loss_out, float* row, void* stream);
/* get_repulsion_loss (loss_utils.py:271-298) value and gradient in one launch (= dispu_repulsion + dispu_repulsion_grad): out [rows]
 * per-point hinge sums, dpred [rows, 3] accumulates scale * d loss / d pred (atomics).  ns == 20. */
int dispu_repulsion_loss_grad(long rows, int n_per_cloud, int ns, float h, float scale, const float* pred, const int* idx, float* out,
                              float* dpred, void* stream);
/* get_uniform_loss (loss_utils.py:238-267; model.py:86) on given seeds, value and gradient in one launch.  pcd [b, n, 3]; seeds
 * [b, npoint] (farthest_point_sample(npoint, pcd)); per level l < nlevels (1..8): ns[l] slots (2..min(64, n)) and levels[l][4] =
 * { r_l = sqrt(p_l R) | e_l = sqrt(pi R^2 p_l / ns_l) | value factor | gradient factor } -- HOST arrays, read when the entry is
 * called (a recorded call keeps the pointers: they must outlive the recording).  For every (cloud, seed) and level: the ball query of
 * dispu_query_ball (r_l, ns_l, same `arith`), every slot's nearest OTHER slot by the squared distance of coordinate differences (the
 * lowest slot on exact ties, tf.nn.top_k's rule), u = sqrt(D + 1e-8), q = (u - e_l)^2 / (e_l + 1e-8);
 *   partial [nlevels, b * npoint]  = value factor * sum of q over the ball's slots, in slot order (get_uniform_loss = the mean of all
 *                                    partials for the value factor (100 p_l)^2 / ns_l);
 *   dpcd [b, n, 3] (may be NULL)  += gradient factor * ((u - e_l) / ((e_l + 1e-8) u)) * 2 (x_a - x_c) at row a, the negative at the
 *                                    partner's row c (atomics; nothing where a == c), seeds / slots / partners held fixed;
 *   idx_out (may be NULL)            the slots, level after level: [b, npoint, ns_0] | [b, npoint, ns_1] | ...; rows without a hit stay
 *                                    untouched (their partial is NaN);  cnt_out [nlevels, b * npoint] (may be NULL) the hit counts.
 * Any n >= 1.  b < 0, n < 1, npoint < 1, nlevels outside 1..8, an ns[l] outside 2..min(64, n) or a NULL required pointer:
 * hipErrorInvalidValue before any device work; b == 0 returns 0 without a launch. */
int dispu_uniform_loss_grad(int b, int n, int npoint, int nlevels, const int* ns, const float* levels, const float* pcd,
                            const int* seeds, float* partial, float* dpcd, int* idx_out, int* cnt_out, int arith, void* stream);
/* dispu_pu_loss_finalize plus the uniform term (model.py:86-87 with the get_uniform_loss line of loss_utils.py:238-267 enabled):
 * out[0..4] as there, out[5] = uniform_w * mean(upart [nlevels, nu]) (dispu_uniform_loss_grad's partials), and out[3] (pu_loss)
 * includes out[5].  One workgroup, fixed summation order. */
int dispu_pu_loss_finalize_u(const float* cd, const float* rep, long nrep, float wf, float rep_w, const float* upart, int nlevels,
                             long nu, float uniform_w, float* out, void* stream);
/* the loss head with the EMD line of DisPU/model.py:77 enabled (`dis_fine_emd = 10.0 * earth_mover(fine, gt, radius)`): the inputs of
 * dispu_pu_loss_finalize_u with upart NULL-able (NULL: no uniform term, out[5] = 0, nlevels / nu ignored) plus emd_cost [b] =
 * dispu_emd_loss_grad's costs, radius [b] (NULL: 1) and m points per cloud.  out[0..2], out[4], out[5] as there;
 * out[6] = dis_fine_emd = emd_w * mean_b(emd_cost[b] / radius[b] / m) (loss_utils.py:170-176);
 * out[3] = pu_loss = ((out[0] + wf * (out[1] + out[6])) + out[2]) [+ out[5] with upart] in fp32, in this order: the term is weighted by
 * weight_fine like dis_fine_cd (the reference never sums it: INTEGRATION.md).  One workgroup, fixed summation order. */
int dispu_pu_loss_finalize_e(const float* cd, const float* rep, long nrep, float wf, float rep_w, const float* upart, int nlevels,
                             long nu, float uniform_w, const float* emd_cost, const float* radius, int b, int m, float emd_w,
                             float* out, void* stream);
/* dst[off ..] = W^T [N][K] for every weight matrix W [K][N] at src[off ..]; desc [count][3] = {off, K, N} (device int32).  The training
 * step's dX = dZ . W^T products read W^T untransposed (the forward GEMM's fast path). */
int dispu_transpose_batched(int count, const int* desc, const float* src, float* dst, void* stream);
/* bf16 ACTIVATION STORAGE of the training step (Trainer(dtype="bf16"), BASELINE configs[4]): the [B*M*16, 128] pair tensors of
 * the PointShuffle2 local cell (h0, h1, their gradients) and the gradient of F' [B*M, 2048] live in HBM as bf16; the entries below
 * take such tensors behind `void*` (strides in ELEMENTS).  storage bits of the GEMMs: 1 = X is bf16, 2 = Z is bf16 (tn only),
 * 4 = Y is written as bf16. */
int dispu_linear_bf16s(int batch, int M, int K, int N, const void* X, long ldx, long sx, const float* W, long ldw, long sw, int transb,
                       const float* bias, int act, void* Y, long ldy, long sy, const float* R1, long ldr1, long sr1, int storage,
                       void* stream);
int dispu_linear_tn_bf16s(int batch, int M, int K, int N, const void* X, long ldx, long sx, const void* Z, long ldz, long sz, float* out,
                          long ldo, long so, int accumulate, float* dbias, float* scratch, long scratch_floats, int storage, void* stream);
int dispu_ps_gather_sub_relu_bf16(long rows, int n_per_cloud, int k, int c, const int* idx, const float* G, long ldg, const float* A,
                                  long lda, void* X1, long ldx1, void* stream);
int dispu_ps_point_matmul_grad_relu_s(long rows, int k, int c, int t_n, const void* X2, long ldx2, const float* wv, const void* dout,
                                      long ldo, void* dX2, long lddx2, float* dwv, int bf16_storage, void* stream);
int dispu_ps_conv0_gather_grad_s(long rows, int n_per_cloud, int k, int c, const int* idx, const int* off, const int* inv, const void* dh0,
                                 long ldz, int dh0_bf16, const float* Gm, long ldgm, const float* Am, long ldam, float* dG, long ldg,
                                 float* dAneg, long lda, void* stream);
/* dispu_ps_point_matmul_grad with conv1's ReLU gradient folded in: dX2 is zero where X2 <= 0. */
int dispu_ps_point_matmul_grad_relu(long rows, int k, int c, int t_n, const float* X2, long ldx2, const float* wv, const float* dout,
                                    long ldo, float* dX2, long lddx2, float* dwv, void* stream);

/* ---- training data path (DisPU/dataset.py:118-143; Common/point_operation.py:32-123: numpy on the host in the
 * reference) ------------------------------------------------------------------------------------------------------
 * out[b,i,:] = ((in[b,i,:] + noise[b,i,:]) . rot[b]) * scale[b] + shift[b]   (jitter -> rotate -> scale [-> shift]);
 * rot [b,9] row-major with p' = p . R as np.dot(points, R); noise [b,n,3] and shift [b,3] may be NULL. */
int dispu_augment(int b, int n, const float* in, const float* noise, const float* rot, const float* scale,
                  const float* shift, float* out, void* stream);

/* One training batch in ONE launch, every random draw made on the device.  Replaces, per batch, the host side of
 * DisPU/dataset.py:113-143 (Fetcher.next_batch) and what it calls in Common/point_operation.py: nonuniform_sampling :10-18,
 * rotate_point_cloud_and_gt :32-71 (z rotation), jitter_perturbation_point_cloud :74-86, random_scale_point_cloud_and_gt :107-123.
 * Patch i of the batch is POSITION p = start + i of the epoch: it uses dataset row perm[p] and Philox4x32-10 draws keyed by
 * (seed, epoch, p) -- independent of B and of the launch shape (counter layout: DESIGN.md, "Train phase").
 *   gt_data [L, G, 3]   normalised ground-truth patches, resident;  perm [L] int32 row permutation, resident
 *   input_data          NULL: the input is a sub-sample of P of the G ground-truth points, indices ascending (`random=True`);
 *                       else [L, P, 3]: the input is row perm[p] of it (`random=False`)
 *   augment != 0        clipped Gaussian jitter (input only), z rotation, scale in [0.8, 1.2] (both clouds): the arithmetic of
 *                       dispu_augment on the device's own draws, bit for bit
 *   input [B, P, 3], gt [B, G, 3], radius [B] (ones)                         outputs
 *   status [2] int32    status[0] = 1: the bounded candidate loop ran out (DISPU_SAMPLER_MAX_ROUNDS rounds of 64 draws; the set was
 *                       filled with the lowest unused indices);  status[1] = 1: a perm entry outside [0, L) (row 0 was used).
 *                       Only ever SET here (plain stores, no atomics): the caller clears it and reads it when it likes.
 *   idx_out [B, P], rot_out [B, 9], scale_out [B], noise_out [B, P, 3], raw_out [B, 4] (the patch-scalar Philox block)
 *                       verification outputs, each may be NULL (noise_out needs augment != 0).
 * Refused before any launch (hipErrorInvalidValue): P > G, G > DISPU_SAMPLER_MAX_G (membership bitmap + owner slots live in LDS),
 * start + B > L, a missing required pointer, augment with jitter_clip <= 0. */
#define DISPU_SAMPLER_MAX_ROUNDS 4096
#define DISPU_SAMPLER_MAX_G 8192
int dispu_sample_batch(int L, int G, int P, const float* gt_data, const float* input_data, const int* perm, int start, int B,
                       unsigned long long seed, int epoch, float jitter_sigma, float jitter_clip, int augment, float* input, float* gt,
                       float* radius, int* status, int* idx_out, float* rot_out, float* scale_out, float* noise_out,
                       unsigned int* raw_out, void* stream);

/* ---- whole-cloud inference glue (DisPU/model.py:306-381, Common/pc_util.py:83-92,147-161; host numpy/sklearn in
 * the reference, one patch at a time) -------------------------------------------------------------------------- */
/* extract_knn_patch: for each of m queries the k nearest of the cloud's n points (k up to n; n > 8192: the radix-select kernel, k <= 4096), ascending
 * squared distance (plain arithmetic), ties -> lower index.  idx [b, m, k]. */
int dispu_knn_patch(int b, int n, int m, int k, const float* cloud, const float* queries, int* idx, void* stream);
/* normalize_point_cloud per patch: out = (in - mean) / max|in - mean|; centroid [b,3], furthest [b]. */
int dispu_normalize_patches(int b, int n, const float* in, float* out, float* centroid, float* furthest, void* stream);
/* out = centroid + in * furthest per patch (model.py:310-311). */
int dispu_denormalize_patches(int b, int m, const float* in, const float* centroid, const float* furthest, float* out,
                              void* stream);
/* Ragged batches of whole clouds (model.py:315-381 for C clouds of different sizes at once; pc_util.py:83-92,147-161).  cloud / in
 * [sum n_c, 3] packs the clouds, off [C+1] (device int32, off[0] = 0) the segment offsets, off_host the same offsets in host memory
 * (tiers, LDS sizes, validation; never read on the device).
 * dispu_knn_patch_segments: extract_knn_patch per segment; queries [sum m_c, 3] packed by qoff / qoff_host, idx [sum m_c, k] local
 * indices.  Bit-identical to dispu_knn_patch on each cloud alone (segments above 8192 points: the radix-select kernel, k <= 4096);
 * each query sorts over its own segment's padded size.  C <= 65535.
 * dispu_normalize_segments: normalize_point_cloud over each whole segment, centroid [C,3], furthest [C]; the sequential float32 mean
 * of dispu_normalize_patches, so each segment is bit-identical to it on that cloud alone.
 * (Gathers take global indices through dispu_gather_point at b = 1; de-normalisation is dispu_denormalize_patches with per-patch
 * copies of a cloud's centroid and radius.) */
int dispu_knn_patch_segments(int C, const int* off, const int* qoff, const int* off_host, const int* qoff_host, int k, const float* cloud,
                             const float* queries, int* idx, void* stream);
int dispu_normalize_segments(int C, const int* off, const int* off_host, const float* in, float* out, float* centroid, float* furthest,
                             void* stream);

/* ---- evaluator: point-to-surface distance and disk uniformity (evaluation_code/evaluation.cpp, a CGAL + pthreads tool in the
 * reference, and evaluate.py:53-101) ------------------------------------------------------------------------------------------- */
/* Per point, the closest point on a triangle mesh: replaces evaluation.cpp:202-214 (AABB-tree `locate`, `point`, squared_distance).
 * Face layout (dis-pu_amd/mesh.py:Mesh builds it once per mesh): tris [F][12] fp32 = v0.xyz, 0, v1.xyz, 0, v2.xyz, 0 in tile order,
 * face_ids [F] the original face index of each entry, tile_box [ceil(F/64)][8] = min.xyz, 0, max.xyz, 0 of the DISPU_MESH_TILE
 * consecutive entries of each tile (NULL: brute force).  Outputs dist [n] (Euclidean), proj [n][3] (closest surface point), face [n]
 * (original index).  The smallest fp32 squared distance wins, an exact tie goes to the lowest original face index; the winner's
 * point and distance are recomputed in fp64.  A tile is skipped only when its conservative lower bound is strictly above the best
 * squared distance found so far, so the pruned path and DISPU_MESH_BRUTE_FORCE give bit-identical outputs. */
int dispu_point_to_mesh(int n, const float* points, int F, const float* tris, const int* face_ids, const float* tile_box, float* dist,
                        float* proj, int* face, int flags, void* stream);
/* Disk membership, evaluation.cpp:68-115 with the EUCLIDEAN distance between the seed and the projected point (CGAL's pre-filter at
 * :95; CGAL then tests the geodesic distance, :98-100).  Point q is in disk (i, j) iff d2 <= fl32(r_j * r_j), d2 = (dx*dx + dy*dy) + dz*dz,
 * dx = points[q].x - seeds[i].x.  Two calls: dispu_disk_count writes offsets [S*R + 1] (int64 CSR row starts, rows seed-major
 * i*R + j = the line order of `_disk_idx.txt`; two launches: counts, then an in-place scan); the caller reads offsets[S*R] back to
 * size `members`, and dispu_disk_fill writes every row's point indices in ascending order (CGAL's pred_iter loop). */
int dispu_disk_count(int S, int n, int R, const float* seeds, const float* points, const float* radii, long long* offsets,
                     void* stream);
int dispu_disk_fill(int S, int n, int R, const float* seeds, const float* points, const float* radii, const long long* offsets,
                    int* members, void* stream);
/* Disk uniformity, evaluate.py:53-101 (analyze_uniform) over a CSR of S*R disks (from dispu_disk_fill or a parsed `_disk_idx.txt`;
 * members must index points [n][3]).  Per radius j, with expect = pct[j] * N: disks of count c < 5 are skipped; a kept disk adds
 * (c - expect)^2 / expect * mean_a((nn_a - expect_d)^2 / expect_d), expect_d = sqrt(2 (pi r_j^2 / c) / 1.732), nn_a = the distance to
 * the nearest OTHER member (sklearn's 2-NN: 0 for duplicates); out[j] (fp64) = the mean over kept disks, NaN if none.  Any disk size;
 * the reductions run in a fixed order (bit-identical run to run).  scratch >= dispu_disk_uniformity_scratch_bytes(S, R). */
size_t dispu_disk_uniformity_scratch_bytes(int S, int R);
int dispu_disk_uniformity(int S, int R, int n, const float* points, const long long* offsets, const int* members, const double* radii,
                          const double* pct, int N, void* scratch, size_t scratch_bytes, double* out, void* stream);
/* Exact geodesic disks, evaluation.cpp:85-115 (Surface_mesh_shortest_path, one source per seed; shortest_distance_to_source_points for
 * every projected point that passes the straight-line pre-filter at :95).  Chen-Han / Xin-Wang window propagation in parallel
 * rounds, one workgroup per seed, fp64 throughout (csrc/geodesic.hip).  Mesh tables (dis-pu_amd/mesh.py:geodesic_tables): verts
 * [V][3] f64, faces [F][3], twin [F][3] (g*3 + k' of the other face on edge k, -1 on a boundary), edge_geo [F][3][3] f64 (L, cx, cy of
 * edge k), pseudo [V] (1: saddle or boundary vertex), fan_off [V+1] i64 / fan (corners f*3 + j around each vertex).
 * Seeds: seed_face [S], seed_bary [S][3] f64 (zeros allowed: a seed on an edge or a vertex).  Targets: points [n][3] with their faces
 * point_face [n] (dispu_point_to_mesh's proj / face); the candidates of seed i are cand[cand_off[i] .. cand_off[i+1]) (ascending point
 * indices, e.g. dispu_disk_count / dispu_disk_fill at max_dist widened by a few ulps).  Writes dist[c] (fp64, aligned with cand) = the
 * geodesic distance from seed i to point cand[c], +inf above max_dist, and status[i] = 0, or 1 / 2 when the seed's window arena
 * (window_cap windows) or its vertex table (dispu_geodesic_hash_slots(window_cap) slots) overflowed: that seed's distances are then
 * not written and the caller reruns it with a larger window_cap.  scratch >= dispu_geodesic_scratch_bytes(S, window_cap), refused
 * (and left untouched) if smaller.  Bit-identical run to run. */
size_t dispu_geodesic_scratch_bytes(int S, int window_cap);
int dispu_geodesic_hash_slots(int window_cap);
int dispu_geodesic_distances(int S, const int* seed_face, const double* seed_bary, const double* verts, const int* faces, const int* twin,
                             const double* edge_geo, const int* pseudo, const long long* fan_off, const int* fan, int n, const float* points,
                             const int* point_face, const long long* cand_off, const int* cand, double max_dist, int window_cap,
                             void* scratch, size_t scratch_bytes, double* dist, int* status, void* stream);
/* Geodesic disk membership from those distances, evaluation.cpp:98-100: point cand[c] is in disk (i, j) iff dist[c] <= (double)radii[j].
 * The same two-call CSR as dispu_disk_count / dispu_disk_fill: offsets [S*R + 1] int64, rows seed-major i*R + j, members ascending. */
int dispu_geodesic_disk_count(int S, int R, const long long* cand_off, const double* dist, const float* radii, long long* offsets,
                              void* stream);
int dispu_geodesic_disk_fill(int S, int R, const long long* cand_off, const int* cand, const double* dist, const float* radii,
                             const long long* offsets, int* members, void* stream);
/* per-row mean and standard deviation (ddof 0) of x[b, n] over the non-NaN entries, fp64: out [b][2] (np.nanmean / np.nanstd of
 * evaluate.py:158-159,202-203 on the P2F distances; the std companion of dispu_row_mean_max). */
int dispu_row_mean_std(int b, int n, const float* x, double* out, void* stream);

/* ---- meshes -> data: surface samples, Poisson-disk selection (no reference counterpart: the reference's patches and test clouds were
 * Poisson-disk sampled upstream with tools in neither tree; the yardstick is the sequential float64 / numpy restatement in
 * tests/mesh_sample_oracle.py, reproduced bit for bit).  dis-pu_amd/mesh_sample.py, csrc/mesh_sample.hip, csrc/poisson_disk.hip -------- */
/* count samples on the surface of a triangle mesh, face chosen with probability proportional to its area, uniform inside the face.
 * verts [V,3] f32, faces [F,3] i32, cum [F+1] f64 = the normalised cumulative face areas (cum[0] = 0).  Sample i draws Philox4x32-10
 * with counter (i lo, i hi, 0, 0xD15C5A3D) and key (seed lo, seed hi) -> w0..w3:  u = ((w0 << 21) | (w1 >> 11)) 2^-53;  face = the largest
 * f in [0, F) with cum[f] <= u (a face of zero area is never drawn);  r1 = (w2 >> 8) 2^-24, r2 = (w3 >> 8) 2^-24, s = sqrt((double)r1),
 * b = (1 - s, s (1 - r2), s r2);  point = (b0 v0 + b1 v1) + b2 v2 per coordinate in fp64, no contraction, rounded to fp32 once.
 * -> points [count,3] f32, face [count] i32, bary [count,3] f64 (NULL: not written).  One thread per sample and no state: sample i does
 * not depend on count or on the launch shape. */
int dispu_mesh_sample(int V, int F, const float* verts, const int* faces, const double* cum, int count, unsigned long long seed,
                      float* points, int* face, double* bary, void* stream);
/* Greedy dart throwing over points [b,n,3] in index order: keep[i] = 1 iff no j < i has keep[j] and d2(p_i, p_j) < fl32(r r), with
 * d2 = (dx dx + dy dy) + dz dz in fp32 (DISPU_ARITH_PLAIN) and a strict comparison; radius [b] per cloud, r <= 0 keeps everything.
 * Computed in parallel rounds, one workgroup per cloud over a 32^3 grid (csrc/poisson_disk.hip); the result is the sequential one
 * whatever the timing, and identical from run to run (no float atomics).  keep [b,n] u8, count [b] i32 = kept points per cloud,
 * status [b] i32: bit 0 = the round loop hit DISPU_POISSON_MAX_ROUNDS (a dependency chain that long; the outputs are then incomplete).
 * Coordinates must be finite.  scratch >= dispu_poisson_disk_scratch_bytes(b, n), 16-byte aligned; refused (hipErrorInvalidValue) when
 * smaller, and for n > DISPU_POISSON_MAX_N.
 * DISPU_POISSON_MAX_N: a cloud lives in ONE workgroup whose LDS holds the 16-bit offsets of the 32^3 cells (64 KB), one state byte per
 * point and one selection bit per point: 128 + 65536 + n + n / 8 bytes.  The 16-bit offsets bound n below 65536; 49152 (6 x 8192: up to
 * 6 x oversampling of an 8192-point cloud) needs 118 KB of the 160 KB a CU of this part has.  Larger clouds take the
 * device-wide cell tier below (dispu_poisson_cells_keep / _select), which returns the same bytes. */
#define DISPU_POISSON_MAX_N 49152
#define DISPU_POISSON_MAX_ROUNDS 256
size_t dispu_poisson_disk_scratch_bytes(int b, int n);
int dispu_poisson_disk_keep(int b, int n, const float* points, const float* radius, unsigned char* keep, int* count, void* scratch,
                            size_t scratch_bytes, int* status, void* stream);
/* Exactly m points per cloud: bisection of the radius on the device (lo = 0, hi = r_hi[c]; steps times mid = 0.5f (lo + hi), the keep
 * count at mid >= m ? lo = mid : hi = mid, fp32), then idx [b,m] i32 = the first m kept indices (ascending) at r = lo,
 * r_out [b] = lo, count_out [b] = the keep count at lo (>= m; the surplus count - m is what the resolution of `steps` leaves).  Any
 * r_hi is legal, a poor one only costs resolution (the natural one: the hexagonal-lattice spacing sqrt(2 area / (sqrt 3 m))).
 * One launch, no host readback.  status as above (bit 1: fewer than m indices were written, only together with bit 0).  1 <= m <= n. */
int dispu_poisson_disk_select(int b, int n, int m, int steps, const float* points, const float* r_hi, int* idx, float* r_out,
                              int* count_out, void* scratch, size_t scratch_bytes, int* status, void* stream);
/* every row of idx [b,k] i32 ascending, in place (k <= 4096; one workgroup per row, bitonic network in LDS).  dispu_knn_patch returns
 * a region's points by distance; the greedy order of the selection must be the sample order, i.e. the index order. */
int dispu_sort_rows_i32(int b, int k, int* idx, void* stream);
/* The same selection for clouds of any size: the device-wide cell tier (csrc/poisson_disk_cells.hip, dis-pu_amd/poisson_cells.py).  The
 * definition is dispu_poisson_disk_keep's, word for word (index order, d2 = (dx dx + dy dy) + dz dz in fp32, DISPU_ARITH_PLAIN, strict
 * comparison, r <= 0 keeps everything), and the result is the sequential one bit for bit, whatever the timing, the launch shape or the
 * packing, and identical from run to run (no float atomics).  Input: a packed ragged batch of C segments (1 <= C <= 65535, 1 .. 2^24
 * points each, fewer than 2^31 in all) in points [off[C],3]; off [C+1] on the device, off_host the same on the host; radius [C] on the
 * device, one per segment.  Per segment a uniform grid of cell side max(r, extent / 1024) (1 + 2^-10), keys (segment, z, y, x) through
 * dispu_radix_sort_pairs' sorter, the 9 neighbour ranges kept per occupied cell; one launch per round over the still-active points,
 * states updated in place (the kernel file says why that is safe), at most DISPU_POISSON_MAX_ROUNDS launches per evaluation.
 * keep [off[C]] u8, count [C] i32, rounds (NULL: not written) [1] i32 = the rounds the evaluation took.  status [C] i32, written by
 * the call: bit 0 = the segment was still active at the round bound (its outputs are then incomplete), bit 1 (select only) = fewer
 * than m indices were written (only together with bit 0), bit 2 (DISPU_POISSON_CELLS_NONFINITE) = a non-finite coordinate or radius, or an extent beyond the float
 * range (the segment is then not evaluated: its flags are all 1).  The call is synchronous: it reads ONE 4-byte word back per chunk of
 * rounds to stop early.  scratch >= dispu_poisson_cells_scratch_bytes(C, off[C]) (0 for illegal sizes), 16-byte aligned; refused
 * (hipErrorInvalidValue) when smaller, and for offsets that do not start at 0 or do not grow. */
#define DISPU_POISSON_CELLS_NONFINITE 4
size_t dispu_poisson_cells_scratch_bytes(int C, long long total_n);
int dispu_poisson_cells_keep(int C, const int* off, const int* off_host, const float* points, const float* radius, unsigned char* keep,
                             int* count, int* rounds, void* scratch, size_t scratch_bytes, int* status, void* stream);
/* Exactly m_c = moff[c + 1] - moff[c] points per segment (1 <= m_c <= n_c; moff [C+1] on the device, moff_host on the host):
 * dispu_poisson_disk_select's bisection bit for bit, per segment on the device (lo = 0, hi = r_hi[c]; steps times mid = 0.5f (lo + hi),
 * the keep count at mid >= m_c ? lo = mid : hi = mid, fp32), the grid built once for r_hi, all segments in the same launches.
 * idx [moff[C]] i32 = per segment its first m_c kept indices at r = lo, local to the segment, ascending; r_out [C] = lo;
 * count_out [C] = the keep count at lo; rounds (NULL: not written) [steps + 1] i32 = the rounds of every evaluation.  steps >= 0. */
int dispu_poisson_cells_select(int C, const int* off, const int* moff, const int* off_host, const int* moff_host, int steps,
                               const float* points, const float* r_hi, int* idx, float* r_out, int* count_out, int* rounds,
                               void* scratch, size_t scratch_bytes, int* status, void* stream);

/* ---- grid subsampling: libs/cpp_wrappers/cpp_subsampling (compile_op.sh builds it with the other ops), the KPConv voxel-grid
 * subsampler.  dis-pu_amd/grid_subsampling.py, csrc/grid_subsample.hip, csrc/radix_sort.hip; the yardstick is the sequential float32 numpy restatement in
 * tests/grid_subsample_oracle.py, held to outputs recorded from the reference's own function, reproduced bit for bit ------------------- */
/* Stable LSD radix sort of n (key u64, payload u32) pairs by the low `bits` bits of the key (0 <= bits <= 64; the higher bits must be
 * equal in all keys, or the order is the one of the low bits only), 8 bits per pass, ceil(bits / 8) passes; bits = 0 copies.  Equal
 * keys keep their input order: the order std::unordered_map<size_t, SampledData> insertion followed by in-order accumulation has in
 * grid_subsampling.cpp:50-77, which no sort of the reference provides (it has none).  The inputs are only read and must not alias the
 * outputs.  scratch >= dispu_radix_sort_scratch_bytes(n), 16-byte aligned.  0 <= n < 2^31.  A tile is DISPU_RADIX_TILE elements.
 * No kernel waits on another workgroup; integer LDS atomics only; identical bytes from run to run. */
#define DISPU_RADIX_TILE 2048
size_t dispu_radix_sort_scratch_bytes(long long n);
int dispu_radix_sort_pairs(long long n, int bits, const unsigned long long* keys_in, const unsigned int* vals_in,
                           unsigned long long* keys_out, unsigned int* vals_out, void* scratch, size_t scratch_bytes, void* stream);
/* grid_subsampling (grid_subsampling.cpp:5-106, SampledData grid_subsampling.h:10-80, min_point / max_point cloud.cpp:27-67) in two
 * steps over one scratch buffer of dispu_grid_subsample_scratch_bytes(n, fdim, ldim) bytes (16-byte aligned; 0 for illegal sizes).
 * All in fp32, one rounding per operation, divisions correctly rounded:  origin = floor(min * (1.0f / dl)) * dl;  NX = floor((max.x -
 * origin.x) / dl) + 1, NY, NZ likewise;  per point i = floor((p - origin) / dl) per axis, key = iX + NX iY + NX NY iZ (signed: the
 * doubly rounded origin can lie a few ulps above the minimum, a point below it gets cell -1 -- the reference's size_t key wraps modulo
 * 2^64 there, which groups the same points).  Per key: count, the sum of the points and of the features added in ascending point index
 * from 0, one label histogram per label column.  Output row per key, rows in ASCENDING KEY ORDER (the reference: unordered_map order):
 * point * (float)(1.0 / count), features / (float)count, per label column the most frequent label, a tie going to the SMALLEST label
 * (signed; the reference: whichever std::max_element meets first in unordered_map order).
 * plan: points [n,3] f32 -> *m_out = the number of occupied voxels, the sorted order left in scratch for emit.  Synchronous: it reads
 * back the bounds with the non-finite flag, and m (two small device-to-host copies).  *status_out = 0, or a refusal (nothing further is
 * launched, *m_out = 0): DISPU_GRID_NONFINITE a coordinate is NaN or infinite; DISPU_GRID_AXIS_X / _Y / _Z that axis has more than 2^21
 * cells (keys must stay below 2^63; tested in float before any conversion to an integer) -- use a larger dl;
 * DISPU_GRID_TOO_MANY_POINTS n >= 2^31.  grid_out (NULL or 8 doubles): origin x y z, NX, NY, NZ, sort passes, the smallest key.
 * emit: with the same n, points and scratch and plan's m -> out_points [m,3] f32, out_features [m,fdim] f32 (features [n,fdim]),
 * out_classes [m,ldim] i32 (classes [n,ldim]); fdim = 0 / ldim = 0: those pointers are not used.  Asynchronous on the stream.
 * One lane per (voxel, column) walks its run serially (the float order is pinned): a voxel holding all n points costs n serial adds. */
#define DISPU_GRID_NONFINITE 1
#define DISPU_GRID_AXIS_X 2
#define DISPU_GRID_AXIS_Y 3
#define DISPU_GRID_AXIS_Z 4
#define DISPU_GRID_TOO_MANY_POINTS 5
size_t dispu_grid_subsample_scratch_bytes(long long n, int fdim, int ldim);
int dispu_grid_subsample_plan(long long n, const float* points, float dl, void* scratch, size_t scratch_bytes, int* m_out, int* status_out,
                              double* grid_out, void* stream);
int dispu_grid_subsample_emit(long long n, int m, int fdim, int ldim, const float* points, const float* features, const int* classes,
                              void* scratch, size_t scratch_bytes, float* out_points, float* out_features, int* out_classes, void* stream);

/* ---- oriented normals of whole clouds, csrc/normals.hip, dis-pu_amd/normals.py.  The reference has no counterpart: it reads and writes
 * bare x y z.  The neighbourhood rule is pc_util.py:83-92's k-NN made deterministic, the rule of dispu_knn_patch_segments: the
 * k' = min(k, n_c) points of the query's own segment with the smallest (d2, local index), d2 = ((dx*dx + dy*dy) + dz*dz) in fp32
 * (DISPU_ARITH_PLAIN), the point itself and duplicates included.  The yardstick is tests/normals_oracle.py. -------------------------- */
/* cloud [sum n_c, 3] packs C <= 65535 clouds of 1 <= n_c <= 2^24 points, off [C+1] device offsets, off_host the same on the host (never
 * read on the device); 4 <= k <= 32.  The pre-pass of dispu_fps_cells (Morton cells of 64 sorted points with boxes) makes the exact
 * search nearly linear: one wave per cell, a cell is visited only if its box-to-box lower bound does not exceed the wave's largest
 * k-th distance.  With q_j = p_j - p_i over the neighbourhood, mu = sum q_j / k', Cov = sum q_j q_j^T / k' - mu mu^T in double,
 * eigenvalues l0 <= l1 <= l2 (cyclic Jacobi in double):  normal [sum n_c, 3] = a unit eigenvector of l0 as fp32;  variation
 * [sum n_c] (or NULL) = fp32(max(l0, 0) / (l0 + l1 + l2));  k' < 3 or l2 = 0: normal (0, 0, 0), variation -1.
 * Sign: orient_mode 0: the component of largest magnitude is positive (ties: the lowest axis);  1: orient [sum n_c, 3], one direction
 * per point, the normal is flipped where the dot product is negative, a dot product of exactly 0 keeps the mode-0 sign;  2: orient
 * [C, 3], one viewpoint per segment, direction = viewpoint - p.  orient may be NULL for mode 0.
 * idx_out [sum n_c, k] (or NULL): the neighbours' local indices in ascending (d2, index) order, rows with k' < k padded with -1.
 * status [C] (device): 0, or 1 for a segment that holds a NaN or an infinite coordinate, for which NO output is written.
 * scratch: 16-byte aligned, scratch_bytes >= dispu_pca_normals_scratch_bytes(C, off_host, k) (0 for an illegal C, k, offsets or a
 * segment above 2^24 points); the library never allocates, and a refusal (hipErrorInvalidValue: k outside 4 .. 32, illegal offsets,
 * a scratch that is NULL or too small) touches no output.  Identical bytes from run to run. */
size_t dispu_pca_normals_scratch_bytes(int C, const int* off_host, int k);
int dispu_pca_normals_segments(int C, const int* off, const int* off_host, int k, const float* cloud, int orient_mode, const float* orient,
                               float* normal, float* variation, int* idx_out, int* status, void* scratch, size_t scratch_bytes,
                               void* stream);

/* ---- outlier removal for whole clouds, csrc/outliers.hip, dis-pu_amd/outliers.py: the statistical and the radius filter.  The reference
 * has no counterpart.  Batches as for dispu_pca_normals_segments: cloud [sum n_c, 3] packs C <= 65535 clouds of 1 <= n_c <= 2^24 points,
 * off [C+1] on the device, off_host the same on the host; d2 = ((dx*dx + dy*dy) + dz*dz) in fp32 (DISPU_ARITH_PLAIN); neighbourhoods
 * never cross segments.  status [C] (device): 0, or 1 for a segment that holds a NaN or an infinite coordinate, for which nothing else
 * is written.  Every scratch is 16-byte aligned and at least its *_scratch_bytes (0 for illegal arguments); the library never
 * allocates; a refusal (hipErrorInvalidValue) touches no output.  Ordinary stores, no float atomics, identical bytes from run to run.
 * The yardstick is tests/outliers_oracle.py.  Additions only: dispu_version() stays 5. ------------------------------------------------- */
/* The mean distance of every point to its k nearest other points, 1 <= k <= 31.  For point i of a segment of n points take the
 * k' = min(k + 1, n) smallest keys (d2, local index), the point itself included (the rule of dispu_pca_normals_segments at k + 1);
 * s = sum_j sqrt((double)d2_j), added in ascending rank in double;  mean_dist [sum n_c] = (float)(s / max(k' - 1, 1)).  The point's own
 * entry adds 0; where k + 1 duplicates of lower index push it out every term is 0 anyway.  Equal d2 give equal terms: no dependence on
 * tie order.  n = 1 gives 0.  sqrt and / are IEEE double: the value can be reproduced bit for bit.  The search is the cell-pruned exact
 * k-NN of the normals (csrc/knn_cells.h); no [n, k] tensor reaches memory. */
size_t dispu_knn_mean_dist_scratch_bytes(int C, const int* off_host, int k);
int dispu_knn_mean_dist_segments(int C, const int* off, const int* off_host, int k, const float* cloud, float* mean_dist, int* status,
                                 void* scratch, size_t scratch_bytes, void* stream);
/* count [sum n_c] = min(cap, #{ j != i in the segment : d2_ij <= r2 }), r2 = radius * radius rounded once in fp32, the boundary
 * inclusive; radius finite and > 0, cap >= 1 (INT_MAX: exact counts).  Duplicates of a point count as its neighbours.  One wave per
 * Morton cell; a cell is skipped when its box-to-box (or, for every lane, point-to-box) lower bound exceeds r2, and the walk ends once
 * every query of the wave has reached cap. */
size_t dispu_radius_count_scratch_bytes(int C, const int* off_host);
int dispu_radius_count_segments(int C, const int* off, const int* off_host, float radius, int cap, const float* cloud, int* count,
                                int* status, void* scratch, size_t scratch_bytes, void* stream);
/* stats [C, 3] doubles = (mu, sigma, mu + ratio * sigma) of the stored fp32 mean_dist values of each segment, in double:
 * mu = sum d / n,  sigma = sqrt(sum (d - mu)^2 / max(n - 1, 1)), two passes, in a summation order that depends on n alone.
 * status [C]: as dispu_knn_mean_dist_segments wrote it; a flagged segment is skipped (its stats row is not written).  ratio finite. */
int dispu_outlier_threshold_segments(int C, const int* off, const int* off_host, const float* mean_dist, const int* status, double ratio,
                                     double* stats, void* stream);
/* Stable compaction.  The keep flag of point i of segment c (global row g) by rule:  0: ((const int*)src)[g] != 0;  1:
 * (double)((const float*)src)[g] <= stats[c][2] (src = mean_dist);  2: ((const int*)src)[g] >= min_neighbors (src = count).  status
 * (or NULL): a segment with status[c] != 0 keeps nothing.  out_points [kept, 3] (or NULL) the kept points in input order, out_index
 * [kept] int32 their local indices, ascending per segment, new_off [C+1] the offsets of the kept segments (new_off[C] = kept; read it
 * back to know how many rows were written; outputs must hold sum n_c rows).  stats is read by rule 1 only, min_neighbors by rule 2. */
size_t dispu_compact_scratch_bytes(int C, const int* off_host);
int dispu_compact_segments(int C, const int* off, const int* off_host, const float* cloud, int rule, const void* src, const double* stats,
                           int min_neighbors, const int* status, float* out_points, int* out_index, int* new_off, void* scratch,
                           size_t scratch_bytes, void* stream);

/* ---- density-based clustering of whole clouds (exact DBSCAN), csrc/cluster.hip, dis-pu_amd/clusters.py.  The reference has no
 * counterpart.  Batches, d2, status word, scratch rule and refusals as for the outlier filters above; everything is per segment, fp32.
 *   r2       = eps * eps, rounded once in fp32; eps finite and > 0.
 *   core     point i is core when #{ j in its segment : d2_ij <= r2 }, ITSELF INCLUDED and duplicates counted, is >= min_points
 *            (min_points >= 1; the convention of scikit-learn and Open3D).
 *   clusters the connected components of the graph on the core points with an edge wherever d2 <= r2 (d2 is symmetric bit for bit).
 *   ids      0, 1, ... in ascending order of the cluster's smallest core input index.
 *   border   a non-core point with a core point at d2 <= r2 takes the label of the core point with the smallest (d2 bits, input
 *            index); every other non-core point is noise, label -1.  A non-core point never joins two clusters.
 * The labels are a pure function of the input, so the bytes are identical from run to run although the components are found with
 * integer atomics (min, add, or) whose order is free; no float atomics.  Every device loop is capped and none waits for another
 * thread; the capped passes are launched a fixed number of times and return at once when the launch before left nothing to do.
 * labels [sum n_c] int32 in input order;  core_or_null [sum n_c] bytes, 1 for a core point;  sizes_or_null [sum n_c] int32: the entry
 * zero-fills it, then sizes[off[c] + k] = the number of points labelled k in segment c (border points included), k < nclusters[c];
 * nclusters [C].  status [C] (device): 0, or 1 for a segment that holds a NaN or an infinite coordinate, or 2 when a capped loop was
 * still short after the last launch (not reachable by the bounds in csrc/cluster.hip; the caller must treat it as an error); nothing
 * else is written for a segment with status != 0.  Asynchronous: no read-back, no synchronisation.
 * scratch: its first DISPU_CLUSTER_HEAD_INTS ints hold afterwards [0, 4) whether link launch 1 .. 4 ran short of a cap (so launch
 * j + 1 did work iff [j - 1] != 0; launch 1 always works), [4, 8) the same for the four flatten launches, [8] the clusters of the batch.
 * The yardstick is tests/cluster_oracle.py.  Additions only: dispu_version() stays 5. ------------------------------------------------- */
#define DISPU_CLUSTER_HEAD_INTS 16
size_t dispu_cluster_scratch_bytes(int C, const int* off_host);
int dispu_cluster_segments(int C, const int* off, const int* off_host, float eps, int min_points, const float* cloud, int* labels,
                           unsigned char* core_or_null, int* sizes_or_null, int* nclusters, int* status, void* scratch,
                           size_t scratch_bytes, void* stream);
/* Keep flags for the `keep` largest clusters of every segment among those of size >= min_size, 1 <= keep <= 32, min_size >= 1: the
 * clusters ordered by size descending, then id ascending.  labels, sizes, nclusters, status as dispu_cluster_segments wrote them.
 * flags [sum n_c] int32: 1 for a point whose cluster is kept, else 0 (noise, and every point of a segment with status != 0): the src
 * of dispu_compact_segments at rule 0.  One workgroup per segment, `keep` rounds of a maximum taken in a fixed order. */
int dispu_cluster_select_segments(int C, const int* off, const int* off_host, const int* labels, const int* sizes, const int* nclusters,
                                  const int* status, int keep, int min_size, int* flags, void* stream);

/* ---- exact k-NN from one cloud into another, and per-point attributes carried across it: csrc/attributes.hip, dis-pu_amd/attributes.py.
 * The reference interpolates over the three neighbours of a brute-force search (Common/pointnet_util.py:204-208); this is that
 * interpolation at any k <= 32 on exact neighbours, for clouds of scan size.  C <= 65535 segments; segment c has q_c queries and m_c
 * reference points, 1 <= q_c, m_c <= 2^24; queries [sum q_c, 3] and refs [sum m_c, 3] are packed, qoff / roff [C+1] device offsets,
 * qoff_host / roff_host the same on the host; neighbourhoods never cross segments.  The neighbour rule is the project's: for query i of
 * segment c the k' = min(k, m_c) reference points of segment c with the smallest (d2 bits, local reference index),
 * d2 = ((dx*dx + dy*dy) + dz*dz) in fp32 (DISPU_ARITH_PLAIN); a reference point equal to the query counts like any other; 1 <= k <= 32.
 * Both sides go through the Morton-cell pre-pass of dispu_fps_cells; one wave per cell of 64 queries walks the reference segment's box
 * table and skips a cell only when its lower bound exceeds the k-th distance, so the result is exact whatever the geometry.
 * status [C] (device): 0, or 1 for a segment whose queries or references hold a NaN or an infinite coordinate, for which nothing else is
 * written.  scratch: 16-byte aligned, at least dispu_knn_cross_scratch_bytes (0 for an illegal C, illegal offsets or a segment above
 * 2^24 points); the library never allocates; a refusal (hipErrorInvalidValue) touches no output.  Ordinary stores, no float atomics,
 * identical bytes from run to run.  The yardstick is tests/attributes_oracle.py.  Additions only: dispu_version() stays 5. ----------- */
size_t dispu_knn_cross_scratch_bytes(int C, const int* qoff_host, const int* roff_host);
/* idx_out [sum q_c, k] int32: the neighbours' local reference indices in ascending key order, -1 beyond k';  d2_out [sum q_c, k] float:
 * their d2, +inf beyond k'.  Either may be NULL, not both.  sum q_c * k >= 2^31 is refused. */
int dispu_knn_cross_segments(int C, const int* qoff, const int* qoff_host, const int* roff, const int* roff_host, int k,
                             const float* queries, const float* refs, int* idx_out, float* d2_out, int* status, void* scratch,
                             size_t scratch_bytes, void* stream);
/* The same search with the transfer done in the kernel: no [sum q_c, k] tensor reaches memory.  feat [sum m_c, F] float row-major,
 * F >= 1 -> out_feat [sum q_c, F];  labels [sum m_c] int32 -> out_labels [sum q_c];  either pair may be NULL, not both.
 * mode 0, inverse-distance weights in double:  w_j = 1.0 / max((double)d2_j, 1e-10),  den = sum_j w_j,  num_f = sum_j w_j *
 * (double)feat[r_j][f], both added in ascending rank over the k' neighbours,  out_feat = (float)(num_f / den); every operation is one
 * IEEE double operation, so the value can be reproduced bit for bit.  mode 1: the row of the rank-0 neighbour.  Labels always take the
 * rank-0 neighbour's label (ties in d2 go to the smallest index).  Feature values are not inspected: a NaN propagates.
 * mode outside {0, 1}, F < 1 or sum q_c * max(F, k) >= 2^31 is refused. */
int dispu_transfer_attributes_segments(int C, const int* qoff, const int* qoff_host, const int* roff, const int* roff_host, int k, int mode,
                                       const float* queries, const float* refs, int F, const float* feat, float* out_feat,
                                       const int* labels, int* out_labels, int* status, void* scratch, size_t scratch_bytes, void* stream);

/* ---- consistent normal orientation, csrc/orient_consistent.hip, dis-pu_amd/normals.py:orient_consistent (Hoppe et al. 1992): the sign
 * is propagated along the minimum spanning forest of the k-NN graph.  The reference has no counterpart.  Batches as for
 * dispu_pca_normals_segments: C <= 65535 clouds of 1 <= n_c <= 2^24 points packed in points / normal_in [sum n_c, 3] and neighbors
 * [sum n_c, k] (int32 LOCAL indices, as dispu_pca_normals_segments' idx_out), 4 <= k <= 32, sum n_c * k < 2^31; off [C+1] on the device,
 * off_host the same on the host.  An entry of neighbors equal to -1 or to its own row is ignored; duplicates are harmless.
 * Edges: the undirected union of the lists.  dot = (nx_u*nx_v + ny_u*ny_v) + nz_u*nz_v in fp32, one rounding per operation
 * (DISPU_ARITH_PLAIN);  w = max(0, 1 - |dot|) in fp32;  s(e) = [dot < 0].  Edges are strictly ordered by (bits of w as unsigned,
 * min(u, v), max(u, v)); under a strict order the minimum spanning forest is unique, so the result does not depend on the algorithm
 * (here: Boruvka rounds with a parity union-find, integer min / max / add atomics only).
 * flip[x] = XOR of s(e) along the forest path from x to its component's anchor, XOR the anchor's own flip.  The anchor is the
 * component's point with the largest (z, y, x), compared as fp32 in that order, ties to the lowest index.  vote 0: the anchor is flipped
 * iff the first non-zero of (nz, ny, nx) of its input normal is negative.  vote 1: of the two global choices for the component the one
 * that flips fewer points with a non-zero normal; on a tie the choice of vote 0.
 * normal_out [sum n_c, 3] = normal_in with its three components negated where flip is set (it must not be normal_in);  flip [sum n_c]
 * bytes;  component [sum n_c] = the lowest local index of the point's component;  n_components [C];  any of the last three may be NULL.
 * status [C] (device): 0, or a sum of 1 (a NaN or an infinite normal), 2 (a neighbour index outside [-1, n_c)), 4 (a pointer-chasing
 * loop reached its iteration cap: cannot happen under the strict order, and nothing ever spins); for a segment with status != 0 no
 * other output is written, and the other segments are exact (an illegal index is never followed).
 * flags: 0, or DISPU_ORIENT_HOST_ROUNDS: end the rounds by one 4-byte read-back per round instead of the device-side counter that
 * makes the remaining launches return at once (same results; the call then synchronises the stream).
 * profile_host: NULL, or DISPU_ORIENT_PROFILE_FLOATS host floats; the call then times its phases with events and synchronises:
 * [0] rounds that hooked an edge, [1] setup ms, [2] propose ms, [3] hook ms, [4] compress ms, [5] finish ms, [6] rounds issued.
 * scratch: 16-byte aligned, at least dispu_orient_consistent_scratch_bytes(C, off_host, k) (0 for an illegal C, k or offsets); the
 * library never allocates; a refusal (hipErrorInvalidValue) touches no output.  Identical bytes from run to run.  The yardstick is
 * tests/orient_oracle.py.  Additions only: dispu_version() stays 5. --------------------------------------------------------------- */
#define DISPU_ORIENT_HOST_ROUNDS 1
#define DISPU_ORIENT_PROFILE_FLOATS 8
size_t dispu_orient_consistent_scratch_bytes(int C, const int* off_host, int k);
int dispu_orient_consistent_segments(int C, const int* off, const int* off_host, int k, const float* points, const float* normal_in,
                                     const int* neighbors, int vote, int flags, float* normal_out, unsigned char* flip, int* component,
                                     int* n_components, int* status, void* scratch, size_t scratch_bytes, float* profile_host,
                                     void* stream);

/* ---- moving-least-squares projection of one cloud onto the surface another describes: csrc/mls_project.hip, dis-pu_amd/mls.py.
 * Queries = references denoises a cloud; an upsampled cloud against its input snaps the output onto the input's surface.  The
 * reference has no counterpart.  Batches, offsets, status and scratch as for dispu_knn_cross_segments; 4 <= k <= 32,
 * 1 <= support <= 4, 1 <= iterations <= 8.  One step, for query x (fp32) of segment c against its m_c reference points P:
 *  1. neighbours: the k' = min(k, m_c) points of P with the smallest (d2 bits, local index), d2 = ((dx*dx + dy*dy) + dz*dz) in fp32
 *     (DISPU_ARITH_PLAIN): the project's rule; a reference point equal to the query counts like any other (d2 = 0).
 *  2. weights, in double: D = the d2 of rank k' - 1, rho2 = (support * support) * D; per neighbour in ascending rank r2 = d2_j / rho2;
 *     w_j = 0 if r2 >= 1, else r = sqrt(r2), w_j = (((1 - r)*(1 - r)) * ((1 - r)*(1 - r))) * (4 r + 1)   (Wendland).
 *  3. fit, in double, around x: u_j = p_j - x (exact);  S0 = sum w_j,  c = (sum w_j u_j) / S0,  Cov = (sum w_j u_j u_j^T) / S0 - c c^T,
 *     sums in ascending rank;  the cyclic Jacobi of dispu_pca_normals_segments (same rotation, at most 12 sweeps, same off-diagonal
 *     drop rule);  e = the normalised eigenvector of the smallest eigenvalue (ties: the lowest column);  l0 <= l1 <= l2 the eigenvalues.
 *  4. the query keeps its position BIT FOR BIT if k' < 3, or fewer than 3 weights are non-zero, or D == 0, or l2 <= 0, or
 *     l1 <= 1e-12 * l2 (collinear neighbours: no plane).
 *  5. otherwise t = (c.x*e.x + c.y*e.y) + c.z*e.z and every coordinate becomes (float)((double)x + t * e): the sign of e cancels.
 * iterations = T repeats the step on the moved fp32 positions against the SAME references (in the self case too: the surface stays
 * fixed), so T iterations equal T calls of one, byte for byte.  The reference pre-pass runs once, the query pre-pass before every
 * iteration on the positions it searches from.
 * out [sum q_c, 3]: the new positions at the queries' rows; it must not overlap queries or refs.  idx_out [sum q_c, k] int32 or NULL:
 * the last iteration's neighbours in ascending key order, -1 beyond k'.  sum q_c * k >= 2^31 is refused.
 * status [C] (device): 0, or 1 for a segment whose queries (at any iteration) or references hold a NaN or an infinite coordinate; the
 * step that finds it and every later one write nothing for that segment.
 * scratch: 16-byte aligned, at least dispu_mls_project_scratch_bytes (both pre-passes, one position buffer, two status rows; 0 for an
 * illegal C, illegal offsets or a segment above 2^24 points); the library never allocates; a refusal (hipErrorInvalidValue) comes
 * before any launch and touches no output.  Ordinary stores, no atomics, identical bytes from run to run.  The yardstick is
 * tests/mls_oracle.py.  Additions only: dispu_version() stays 5. ---------------------------------------------------------------------- */
size_t dispu_mls_project_scratch_bytes(int C, const int* qoff_host, const int* roff_host);
int dispu_mls_project_segments(int C, const int* qoff, const int* qoff_host, const int* roff, const int* roff_host, int k, double support,
                               int iterations, const float* queries, const float* refs, float* out, int* idx_out, int* status,
                               void* scratch, size_t scratch_bytes, void* stream);

/* ---- the signed distance to an oriented cloud (IMLS / Hoppe et al. 1992): csrc/signed_distance.hip, dis-pu_amd/reconstruct.py.  The
 * implicit function the surface reconstruction below contours, at arbitrary positions.  The reference has no counterpart.  Batches,
 * offsets, status and scratch as for dispu_mls_project_segments; normals [sum m_c, 3] are the references' rows, used as given (not
 * normalised; a zero row contributes zero) and must be finite: that is the caller's duty, the entry does not look.  1 <= k <= 32,
 * 1 <= support <= 4.  For query x (fp32) of segment c against its m_c reference points P:
 *  1. neighbours: the k' = min(k, m_c) points of P with the smallest (d2 bits, local index), d2 = ((dx*dx + dy*dy) + dz*dz) in fp32
 *     (DISPU_ARITH_PLAIN): the project's rule.
 *  2. in double, one rounding per operation, in ascending rank: D = the d2 of rank k' - 1, rho2 = (support * support) * D; per
 *     neighbour r2 = d2_j / rho2;  w_j = 0 unless r2 < 1 (so also when D == 0: r2 is a NaN), else r = sqrt(r2),
 *     w_j = (((1 - r)*(1 - r)) * ((1 - r)*(1 - r))) * (4 r + 1)   (Wendland);  u = x - p_j (exact),
 *     g_j = (u.x*n_j.x + u.y*n_j.y) + u.z*n_j.z;  S0 = sum w_j,  S1 = sum w_j * g_j.
 *  3. f = S1 / S0 if S0 != 0, else g_0, the nearest point's tangent plane (k' = 1, coincident or equidistant neighbours, D == 0): f is
 *     always defined.  out[x] = (float)f.
 * Every operation is a correctly rounded IEEE one, so the value can be reproduced bit for bit (tests/reconstruct_oracle.py does).
 * out [sum q_c] must not overlap queries, refs or normals.  status [C] (device): 0, or 1 for a segment whose queries or references hold
 * a NaN or an infinite coordinate; nothing is written for it.  No [q, k] tensor reaches memory.  scratch: 16-byte aligned, at least
 * dispu_signed_distance_scratch_bytes (both pre-passes; 0 for an illegal C, illegal offsets or a segment above 2^24 points); a refusal
 * (hipErrorInvalidValue) comes before any launch and touches no output.  Ordinary stores, no atomics, identical bytes from run to run. */
size_t dispu_signed_distance_scratch_bytes(int C, const int* qoff_host, const int* roff_host);
int dispu_signed_distance_segments(int C, const int* qoff, const int* qoff_host, const int* roff, const int* roff_host, int k, double support,
                                   const float* queries, const float* refs, const float* normals, float* out, int* status, void* scratch,
                                   size_t scratch_bytes, void* stream);

/* ---- rigid registration (ICP) of one cloud onto another: csrc/icp.hip, dis-pu_amd/registration.py.  Brings several scans of one object
 * into one frame.  The reference has no counterpart.  Batches, offsets, status and scratch as for dispu_mls_project_segments: pair c is
 * a SOURCE segment (the queries, q_c points) and a TARGET segment (the references, m_c points); plane mode (mode 1) also takes unit
 * target normals packed like the references (used as given, the caller's duty to keep finite; their sign cancels).  The entry
 * estimates per pair a rigid motion T, [C, 4, 4] double, row-major, last row 0 0 0 1, that maps source coordinates into the target's
 * frame.  Every operation below is one IEEE operation in the order written (the build and the kernels pin fp contract off).
 *  apply      cur[i].x = (float)(((T00*x + T01*y) + T02*z) + T03), likewise y and z with rows 1 and 2, in double from the ORIGINAL
 *             fp32 source point and the current T: never chained from rounded positions, so `aligned` can be recomputed from the
 *             returned T bit for bit.  dispu_rigid_apply_segments is this step alone (out may be points itself).
 *  match      the nearest target point of cur[i] under the project's rule: the smallest (fp32 d2 bits, local index), exactly rank 0
 *             of dispu_knn_cross_segments.  The point is an INLIER iff d2 <= max_d2 (both fp32; +inf: no rejection).
 *  equations  in double, about the origin o = the pair's first target point (row 0 of the target segment):  p = cur[i] - o,
 *             qv = y - o for the matched target point y, d = p - qv, n the normal of y.  Unknowns (w, t) of p -> p + w x p + t.
 *             mode 0 (point to point), three residuals d:   Aww = [[py*py + pz*pz, -(px*py), -(px*pz)], [., px*px + pz*pz, -(py*pz)],
 *               [., ., px*px + py*py]],  Awt = [[0, -pz, py], [pz, 0, -px], [-py, px, 0]],  Att = I,
 *               b = (py*dz - pz*dy, pz*dx - px*dz, px*dy - py*dx, dx, dy, dz),  e = (dx*dx + dy*dy) + dz*dz.
 *             mode 1 (point to plane), one residual r = (dx*nx + dy*ny) + dz*nz:  J = (py*nz - pz*ny, pz*nx - px*nz, px*ny - py*nx,
 *               nx, ny, nz),  A_ij = J_i * J_j,  b_i = J_i * r,  e = r * r.
 *             A point that is no inlier contributes zeros.  The 29 sums -- the 21 upper entries of A row by row, the 6 of b, e and
 *             the inlier count -- are formed per query cell (64 consecutive points of the source's Morton order, one per lane) by
 *             the butterfly v += v[lane ^ o], o = 32, 16, 8, 4, 2, 1, and per pair over the cells: cell j goes to slot j mod 32, every
 *             slot is summed in ascending j, the slots are added in ascending order.  No float atomics.
 *  solve      the pair is DEGENERATE when it has fewer than 3 (mode 0) or 6 (mode 1) inliers, when a pivot of the Cholesky
 *             factorisation of A is <= 1e-12 * its diagonal entry of A or is not finite, or when the solution is not finite: it keeps
 *             its T and freezes.  Otherwise (w, t) = -A^-1 b,  R = I + a [w]x + c [w]x^2 with th = |w|, a = sin th / th,
 *             c = (1 - cos th) / th^2 (for th < 1e-12: a = 1 - th^2 / 6, c = 0.5 - th^2 / 24),  U(x) = R (x - o) + o + t,  T <- U o T:
 *             the rotation R * T_R, the translation ((R * (T_t - o)) + o) + t.
 *  converged  after its update, iff tolerance > 0, |w| <= tolerance and |t| <= tolerance * D, D the diagonal of the target segment's
 *             bounding box in double from its fp32 bounds: the pair freezes.  A frozen pair costs the batch-wide source pre-pass and
 *             the apply only; its waves leave the accumulation after the prologue.
 *  loop       the target pre-pass once; `iterations` times: apply, source pre-pass on cur, accumulate, solve; then the evaluation of
 *             the returned T: apply, pre-pass, accumulate (frozen pairs included), no solve.  iterations = 0 evaluates init.  Every
 *             launch is enqueued up front: the entry neither synchronises nor copies to the host, and k iterations equal k calls of
 *             one, each given the transform of the last as init, byte for byte (at tolerance 0).
 * init [C, 16] double or NULL (identity).  Outputs per pair: transform [C, 16];  aligned [sum q_c, 3] = cur under the returned T (it
 * must not overlap source or target);  inliers [C] int;  rmse [C] double = sqrt(e / inliers), 0 without inliers;  iters [C] int, the
 * updates applied;  flag [C] int: 0 out of iterations, 1 converged, 2 degenerate;  corr [sum q_c] int32 or NULL: the matched target
 * point's local index, -1 for a point that is no inlier.
 * status [C] (device): 0, or 1 for a pair either side of which holds a NaN or an infinite coordinate (at any iteration: a transform
 * that overflows fp32 counts); nothing else is written for such a pair.
 * Refused (hipErrorInvalidValue, before any launch, nothing touched): C or offsets as for dispu_knn_cross_segments, a NULL pointer
 * (corr, init and, in mode 0, target_normals may be NULL), mode outside {0, 1}, iterations outside 0 .. 128, max_d2 NaN or negative,
 * tolerance NaN, negative or infinite, a scratch that is NULL, misaligned or shorter than dispu_icp_scratch_bytes (both pre-passes, cur,
 * two status rows, the working T and state, one row of 32 doubles per source cell; 0 for an illegal C or offsets), aligned overlapping
 * source or target.  Ordinary stores only, identical bytes from run to run.  The yardstick is tests/icp_oracle.py.  Additions only:
 * dispu_version() stays 5. ---------------------------------------------------------------------------------------------------------- */
size_t dispu_icp_scratch_bytes(int C, const int* qoff_host, const int* roff_host);
int dispu_icp_segments(int C, const int* qoff, const int* qoff_host, const int* roff, const int* roff_host, int mode, int iterations,
                       float max_d2, double tolerance, const float* source, const float* target, const float* target_normals,
                       const double* init, double* transform, float* aligned, int* corr, int* inliers, double* rmse, int* iters,
                       int* flag, int* status, void* scratch, size_t scratch_bytes, void* stream);
int dispu_rigid_apply_segments(int C, const int* off, const int* off_host, const float* points, const double* transform, float* out,
                               void* stream);

/* ---- surface reconstruction, the lattice and the contouring: csrc/reconstruct.hip, dis-pu_amd/reconstruct.py:reconstruct_surface.
 * f = 0 of the signed distance above, contoured on a sparse lattice by marching tetrahedra, vertices welded, every order pinned: one
 * cloud per call, the output is unique.  The reference has no counterpart.  The entries are split where a count must reach the host to
 * size the next buffer; each `*_host` count is written after the entry's work is done (the stream is synchronised).
 * Lattice: h = voxel (fp32).  A point's voxel index per axis is floorf(p / h), the division correctly rounded; lattice vertex (i, j, l)
 * sits at ((float)i*h, (float)j*h, (float)l*h), one rounding each.  Indices, after the band, stay in +-(2^20 - 1).  A voxel or vertex
 * is the key ((l + 2^20 - 1) << 42) | ((j + 2^20 - 1) << 21) | (i + 2^20 - 1): ascending keys are ascending (l, j, i), z slowest.
 *   dispu_lattice_voxels    occ_out [<= n]: the sorted unique keys of the voxels that hold a point, *count_host of them.
 *                           *status_host: 0, DISPU_LATTICE_NONFINITE (a NaN or an infinite coordinate) or DISPU_LATTICE_RANGE (an index
 *                           outside +-(2^20 - 1 - band)); then the count is 0.  1 <= n <= 2^24, voxel > 0 and finite, band in 1 .. 3.
 *   dispu_lattice_dilate    act_out [<= nocc * (2 band + 1)^3]: the sorted unique keys of every occupied voxel's Chebyshev neighbours
 *                           within band, the active voxels.  nocc * (2 band + 1)^3 < 2^31.
 *   dispu_lattice_corners   lat_out [<= 8 nvox]: the sorted unique keys of the 8 corners of all active voxels, the lattice vertices,
 *                           *count_host of them;  corner_out [nvox, 8]: the lattice-vertex number of corner b = bx + 2 by + 4 bz of
 *                           every active voxel, by binary search.  8 nvox < 2^31.
 *   dispu_lattice_positions pos_out [nlat, 3]: the vertices' positions.  1 <= nlat <= 2^24 (a query segment holds no more).
 * Values: values [nlat] fp32, f at every lattice vertex (dispu_signed_distance_segments with queries = pos).  A vertex is negative iff
 * f < 0 on the fp32 value; an exact zero is not.
 * Tetrahedra: Kuhn's six per voxel around the diagonal 0 -> 7: for the axis permutations (a, b, c) in lexicographic order (xyz, xzy,
 * yxz, yzx, zxy, zyx) the tetrahedron (0, e_a, e_a + e_b, 7), e = (1, 2, 4); translation-invariant, so neighbouring voxels agree on
 * every shared face.  The edge between tet vertices t_i < t_j has lower endpoint A = t_i and direction code d = t_j - t_i in 1 .. 7;
 * its global identity is slot = 7 * (lattice number of A) + d - 1.
 * Cases: n0 < n1 the positions in the tet of its negative vertices, p0 < p1 of the others.  1 or 3 negative: v the odd vertex,
 * o0 < o1 < o2 the rest, the triangle (E(v,o0), E(v,o1), E(v,o2)).  2 negative: the quad q = (E(n0,p0), E(n0,p1), E(n1,p1), E(n1,p0))
 * as (q0, q1, q2) and (q0, q2, q3).  A triangle's last two vertices are swapped iff its normal (b - a) x (c - a), with every vertex at
 * the MIDPOINT of its edge in the unit cube, does not point from the negative corners' centroid to the positive corners' centroid:
 * a table per (tet, sign mask), never a decision on computed positions.
 *   dispu_contour_count     slot_number [7 nlat]: a slot is used when an emitted triangle references it; the exclusive scan of the used
 *                           flags, so mesh vertices are numbered in ascending (lattice vertex, d);  tri_start [nvox]: the exclusive
 *                           scan of the voxels' triangle counts;  *nverts_host, *nfaces_host the totals.
 *   dispu_contour_emit      verts_out [nverts, 3]: per axis and in double t = fa / (fa - fb), then A + t * (B - A), rounded to fp32,
 *                           always from the lower endpoint A; fa, fb the stored fp32 values (fa < 0 <= fb or the reverse).
 *                           faces_out [nfaces, 3] int32 in the order (active voxel ascending, tet 0 .. 5, triangle 0 .. 1).
 *                           nverts, nfaces >= 1: an empty mesh needs no call.
 * Zero-area faces appear when f is exactly 0 at a lattice vertex or fp32 collapses two vertices; they are kept: they keep the
 * connectivity closed.  Outputs of one entry must not overlap its inputs or each other.  scratch: 16-byte aligned, at least the
 * entry's *_scratch_bytes (0 for illegal sizes); the library never allocates; a refusal (hipErrorInvalidValue: NULL, illegal sizes,
 * short or misaligned scratch, overlap) comes before any launch and touches nothing.  Used flags are plain stores of 1; no float
 * atomics, every loop bounded, ordering by kernel boundaries only, identical bytes from run to run.  The yardstick is
 * tests/reconstruct_oracle.py.  Additions only: dispu_version() stays 5. ------------------------------------------------------------ */
#define DISPU_LATTICE_NONFINITE 1
#define DISPU_LATTICE_RANGE 2
size_t dispu_lattice_voxels_scratch_bytes(long long n);
int dispu_lattice_voxels(long long n, const float* points, float voxel, int band, unsigned long long* occ_out, int* count_host,
                         int* status_host, void* scratch, size_t scratch_bytes, void* stream);
size_t dispu_lattice_dilate_scratch_bytes(long long nocc, int band);
int dispu_lattice_dilate(long long nocc, const unsigned long long* occ, int band, unsigned long long* act_out, long long* count_host,
                         void* scratch, size_t scratch_bytes, void* stream);
size_t dispu_lattice_corners_scratch_bytes(long long nvox);
int dispu_lattice_corners(long long nvox, const unsigned long long* act, unsigned long long* lat_out, int* corner_out,
                          long long* count_host, void* scratch, size_t scratch_bytes, void* stream);
int dispu_lattice_positions(long long nlat, const unsigned long long* lat, float voxel, float* pos_out, void* stream);
size_t dispu_contour_count_scratch_bytes(long long nvox, long long nlat);
int dispu_contour_count(long long nvox, long long nlat, const int* corner, const float* values, unsigned* slot_number, unsigned* tri_start,
                        long long* nverts_host, long long* nfaces_host, void* scratch, size_t scratch_bytes, void* stream);
int dispu_contour_emit(long long nvox, long long nlat, float voxel, const unsigned long long* lat, const int* corner, const float* values,
                       const unsigned* slot_number, const unsigned* tri_start, long long nverts, long long nfaces, float* verts_out,
                       int* faces_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DISPU_HIP_H */
