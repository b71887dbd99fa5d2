/*
 * pn2_abi.h -- C ABI of libpn2_hip.so: the MI355X (gfx950) drop-in for the
 * PointNet++ SA/FP custom ops of isl-org/Open3D-PointNet2-Semantic3D.
 *
 * Every entry point replaces one reference launcher / CPU op; dimension and
 * pointer order are kept identical to the reference launcher it replaces so the
 * mapping is auditable (reference file:line cited per function).  Differences
 * from the reference launchers, all deliberate:
 *   - extern "C", returns int (0 = ok, <0 = PN2_E* argument error, >0 = hipError_t
 *     from the launch) instead of void-with-no-error-check;
 *   - explicit stream (a hipStream_t passed as void*; NULL = the HIP null stream)
 *     instead of the legacy default stream (tf_grouping.cu:141 etc.);
 *   - gradient outputs are zero-filled by the callee with a stream-ordered
 *     memset (the reference does it in the TF op glue: tf_sampling.cpp:236,
 *     tf_grouping.cpp:271, tf_interpolate.cpp:477).
 *
 * Conventions: all tensors dense row-major contiguous DEVICE memory; float =
 * IEEE fp32; indices int32.  The caller owns every buffer (outputs and scratch);
 * the library never allocates, never synchronises and keeps no pointers.  Its only mutable global state besides the
 * documented switch pn2_set_sa_row_packing: per kernel that needs more than 64 KiB of dynamic LDS, an atomic set of the
 * devices on which that kernel's LDS limit has been raised (pn2_allow_lds, csrc/pn2_common.h).  Raising the limit is
 * idempotent and the set is safe from several host threads and several devices.  (The kernel-selection knobs of the A/B
 * scripts exist only in a -DPN2_TUNING_HOOKS build.)
 * Re-entrant; safe from several host threads on different streams, and on any device of the process: an entry point runs
 * on the caller's current device, which must be the device of its buffers and its stream.
 */
#ifndef PN2_ABI_H_
#define PN2_ABI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PN2_ABI_VERSION 2

/* error codes (negative); positive return values are hipError_t */
#define PN2_OK 0
#define PN2_EINVAL (-1)  /* non-positive dimension / bad attribute            */
#define PN2_ENULL (-2)   /* required pointer is NULL                          */
#define PN2_ERANGE (-3)  /* dimension exceeds what the kernel supports        */
#define PN2_EUNSUP (-4)  /* unsupported configuration (e.g. channel widths)   */

/* squared-distance arithmetic, see DESIGN.md "Arithmetic modes".  The reference
 * CUDA build leaves nvcc's --fmad=true default on (tf_ops/CMakeLists.txt:5,13). */
#define PN2_ARITH_STRICT 0  /* (dx*dx + dy*dy) + dz*dz, each op rounded        */
#define PN2_ARITH_FMA 1     /* fma(dz,dz, fma(dx,dx, dy*dy))  (default)        */
#define PN2_ARITH_FMA_ALT 2 /* fma(dz,dz, fma(dy,dy, dx*dx))                   */

int pn2_abi_version(void);
const char *pn2_build_info(void);     /* "gfx950 ..." static string */
const char *pn2_strerror(int code);   /* static string for PN2_E* / hipError_t */

/* ---- sampling (replaces tf_ops/tf_sampling.cu) --------------------------- */

/* farthestpointsamplingLauncher(b,n,m,inp,temp,out)  tf_sampling.cu:218-221,
 * declared tf_sampling.cpp:114.  inp (b,n,3) -> out (b,m) int32; first pick is
 * index 0; tie-break (max dist, k mod 512, k) exactly as the 512-thread
 * reference block produces.  `temp` is the reference's (32,n) float scratch: it
 * is only used when n > PN2_FPS_MAX_REG_POINTS (then it must hold
 * min(b,32)*n floats); may be NULL otherwise.  Requires m >= 1. */
#define PN2_FPS_MAX_REG_POINTS 16384
int pn2_farthest_point_sample(int b, int n, int m, const float *inp, float *temp,
                              int *out, int arith_mode, void *stream);

/* farthest_point_sample + gather_point fused (the layer API always chains them,
 * util/pointnet_util.py:36-37): out (b,m) and new_xyz (b,m,3) = inp[out], bit-identical to the two
 * separate calls. */
int pn2_fps_gather(int b, int n, int m, const float *inp, float *temp, int *out,
                   float *new_xyz, int arith_mode, void *stream);

/* Nested sampling: the SA levels chain farthest_point_sample on each other's output (util/pointnet_util.py:36-37 called
 * by model.py:104-113 with l1_xyz, l2_xyz, l3_xyz).  When inp is the new_xyz of an FPS run over a larger cloud, its rows
 * are that run's picks in pick order and sampling them again retraces the same picks -- idx = 0..m-1 -- unless the parent
 * run met a TIE (two points holding the maximum distance) before step m: only then can this level's tie-break
 * (tf_sampling.cu:153-170: lowest k mod 512, then k, in THIS cloud's numbering) choose differently.
 *   tie_in  (b) int32 or NULL: first tied step of the run that produced inp (0x7fffffff = none).  A cloud with
 *           tie_in[i] >= m gets idx = 0..m-1 and new_xyz = its first m rows, no sampling; any other cloud (and every cloud
 *           when tie_in is NULL) is sampled exactly as pn2_fps_gather does.  The result is bit-identical either way.
 *   tie_out (b) int32 or NULL: this level's record, to be passed as the next level's tie_in.  Ties between points of equal
 *           coordinates do not count until the distance maximum reaches 0 (their twin is then picked too).
 * new_xyz (b,m,3) may be NULL (indices only).  temp as for pn2_farthest_point_sample. */
int pn2_fps_nested(int b, int n, int m, const float *inp, float *temp, int *out, float *new_xyz,
                   const int *tie_in, int *tie_out, int arith_mode, void *stream);

/* In-place reads of a batch that keeps xyz and rgb side by side (model.py:26-29 slices point_cloud (b,n,6) into l0_xyz /
 * l0_points; the reference's TF graph materialises both slices): the *_ld entry points take the ROW STRIDE in floats of such a
 * column block (ld >= 3 resp. >= c; the pointer is the block's first element, rows are ld floats apart, cloud i starts at
 * i * n * ld) and read it where it lies -- same bits as the dense entry point on a copy.  Shapes a strided kernel does not
 * exist for return PN2_EUNSUP (the caller then makes the copy).
 * pn2_fps_nested_ld: pn2_fps_nested for n <= 16384 (the register-resident kernels need no temp). */
int pn2_fps_nested_ld(int b, int n, int m, const float *inp, int ld, int *out, float *new_xyz,
                      const int *tie_in, int *tie_out, int arith_mode, void *stream);

/* The coarse levels of the pyramid in ONE launch (extension; replaces 3 launches per level): for l = 0 .. nlev-1, with the
 * source cloud of level l = the samples of level l-1 (level 0: xyz0 (b,n0,3)):
 *   fps_idx[l] (b,npoint[l]) int32, new_xyz[l] (b,npoint[l],3)   = pn2_fps_nested   (util/pointnet_util.py:36-37)
 *   bq_idx[l] (b,npoint[l],nsample[l]) int32, bq_cnt[l] (b,npoint[l]) or NULL = pn2_query_ball_point(radius[l], nsample[l],
 *                                                                 source cloud, new_xyz[l])      (util/pointnet_util.py:39)
 *   nn_dist[l], nn_idx[l] (b,n_l,3), n_l = points of the source cloud, or NULL = pn2_three_nn(source cloud, new_xyz[l])
 *                                                                 (util/pointnet_util.py:300 of the FP level above it)
 * bit for bit.  npoint / radius / nsample are HOST arrays of nlev entries, fps_idx ... nn_idx HOST arrays of nlev device
 * pointers (nn_dist / nn_idx / bq_cnt may be NULL as a whole or per level).  tie_in (b) or NULL: tie record of the run that
 * produced xyz0 (pn2_fps_nested); tie_out (b) or NULL: the record of the last level.  One workgroup per cloud walks down the
 * levels.  PN2_EUNSUP: n0 > 1024, nlev > 4, npoint[l] > points of its source cloud, or a 3-NN table over more than 256
 * samples -- use the separate entry points. */
int pn2_coarse_geometry(int b, int n0, int nlev, const int *npoint, const float *radius, const int *nsample,
                        const float *xyz0, const int *tie_in, int *const *fps_idx, float *const *new_xyz,
                        int *const *bq_idx, int *const *bq_cnt, float *const *nn_dist, int *const *nn_idx,
                        int *tie_out, int fps_arith_mode, int bq_arith_mode, void *stream);

/* probsampleLauncher(b,n,m,inp_p,inp_r,temp,out)  tf_sampling.cu:212-216, tf_sampling.cpp:72.  inp_p (b,n)
 * non-negative weights, inp_r (b,m) uniforms in [0,1) -> out (b,m) int32: the index at which the running sum of
 * the weights reaches inp_r * total (the reference's exact fp32 summation order and branch-free binary search).
 * temp (b,n) receives the running sums (the reference's scratch tensor). */
int pn2_prob_sample(int b, int n, int m, const float *inp_p, const float *inp_r, float *temp, int *out,
                    void *stream);

/* Farthest point sampling for clouds beyond PN2_FPS_MAX_REG_POINTS (16384 < n <= 131072), same picks as
 * pn2_farthest_point_sample (bit-identical), ~6x faster than its streaming path at n = 65536: the cloud is
 * sorted along a Morton curve into 64-point buckets and a round only revisits the buckets whose bounding box the
 * new pick can reach (exact: skipped buckets provably keep their running minima).  new_xyz (b,m,3) may be NULL.
 * `workspace`: 256-byte aligned device scratch of pn2_fps_large_workspace_bytes(b, n) bytes (replaces `temp`). */
size_t pn2_fps_large_workspace_bytes(int b, int n);
int pn2_fps_large(int b, int n, int m, const float *inp, void *workspace, size_t workspace_bytes, int *out,
                  float *new_xyz, int arith_mode, void *stream);

/* gatherpointLauncher(b,n,m,inp,idx,out)  tf_sampling.cu:222-225, tf_sampling.cpp:158 */
int pn2_gather_point(int b, int n, int m, const float *inp, const int *idx,
                     float *out, void *stream);

/* scatteraddpointLauncher(b,n,m,out_g,idx,inp_g)  tf_sampling.cu:226-229,
 * tf_sampling.cpp:195.  inp_g (b,n,3) is zeroed by the callee first. */
int pn2_gather_point_grad(int b, int n, int m, const float *out_g, const int *idx,
                          float *inp_g, void *stream);

/* ---- grouping (replaces tf_ops/tf_grouping.cu) --------------------------- */

/* queryBallPointLauncher(b,n,m,radius,nsample,xyz1,xyz2,idx,pts_cnt)
 * tf_grouping.cu:138-144, tf_grouping.cpp:72.  xyz1 (b,n,3) dataset, xyz2
 * (b,m,3) queries -> idx (b,m,nsample), pts_cnt (b,m).  First nsample hits in
 * index order with max(sqrtf(d2),1e-20f) < radius; short rows padded with the
 * first hit.  Rows with no hit: idx row = 0, pts_cnt = 0 (the reference leaves
 * the row uninitialised; unreachable when queries are dataset points). */
int pn2_query_ball_point(int b, int n, int m, float radius, int nsample,
                         const float *xyz1, const float *xyz2, int *idx,
                         int *pts_cnt, int arith_mode, void *stream);
/* pn2_query_ball_point with the cloud's rows ld1 floats apart (see pn2_fps_nested_ld); only the shapes the LDS-grid kernel
 * takes (4096 <= n <= 8192, m >= 256, nsample <= 64), else PN2_EUNSUP. */
int pn2_query_ball_point_ld(int b, int n, int m, float radius, int nsample, const float *xyz1, int ld1,
                            const float *xyz2, int *idx, int *pts_cnt, int arith_mode, void *stream);
/* The same operator on an explicitly chosen kernel -- 0 by shape (= pn2_query_ball_point), 1 wave-per-queries scan,
 * 2 lane-per-query scan, 3 LDS grid; a kernel whose preconditions do not hold falls through to the next.  Every kernel
 * returns the same bits; this door lets the parity tests hold each of them to the oracle.  Stateless. */
int pn2_query_ball_point_kernel(int b, int n, int m, float radius, int nsample, const float *xyz1,
                                const float *xyz2, int *idx, int *pts_cnt, int arith_mode, int kernel,
                                void *stream);

/* Multi-radius ball query for MSG set abstraction (util/pointnet_util.py:245-250 calls query_ball_point once per
 * radius on the same xyz / new_xyz): ONE scan of xyz1, every squared distance tested against all thresholds.
 * radii, nsamples: host arrays of nradius (1..3) entries; idx[r] (b,m,nsamples[r]) and pts_cnt[r] (b,m): host
 * arrays of device pointers.  Bit-identical to nradius separate pn2_query_ball_point calls.  PN2_EUNSUP when
 * nradius > 3 or the hit lists do not fit LDS (sum of nsamples > ~130): call pn2_query_ball_point per radius. */
int pn2_query_ball_point_multi(int b, int n, int m, int nradius, const float *radii, const int *nsamples,
                               const float *xyz1, const float *xyz2, int *const *idx, int *const *pts_cnt,
                               int arith_mode, void *stream);

/* selectionSortLauncher(b,n,m,k,dist,outi,out)  tf_grouping.cu:145-149, tf_grouping.cpp:135.
 * dist (b,m,n) -> outi (b,m,n) int32, out (b,m,n): partial selection sort of the first k positions
 * of every row including the reference's swaps (whole rows bit-identical).  n <= 19200. */
int pn2_selection_sort(int b, int n, int m, int k, const float *dist, int *outi, float *out,
                       void *stream);

/* groupPointLauncher(b,n,c,m,nsample,points,idx,out)  tf_grouping.cu:150-154,
 * tf_grouping.cpp:178.  out (b,m,nsample,c). */
int pn2_group_point(int b, int n, int c, int m, int nsample, const float *points,
                    const int *idx, float *out, void *stream);

/* groupPointGradLauncher(b,n,c,m,nsample,grad_out,idx,grad_points)
 * tf_grouping.cu:155-162, tf_grouping.cpp:220.  grad_points (b,n,c) zeroed first. */
int pn2_group_point_grad(int b, int n, int c, int m, int nsample,
                         const float *grad_out, const int *idx, float *grad_points,
                         void *stream);

/* The same gradient with caller-provided scratch (see pn2_three_interpolate_grad_ws): a per-point list of the grouped
 * rows that reference it, then a gather -- no float atomics on large levels.  `workspace`: 4-byte aligned, at least
 * pn2_group_point_grad_workspace_bytes(b, n, m, nsample) bytes. */
size_t pn2_group_point_grad_workspace_bytes(int b, int n, int m, int nsample);
int pn2_group_point_grad_ws(int b, int n, int c, int m, int nsample, const float *grad_out, const int *idx,
                            float *grad_points, void *workspace, size_t workspace_bytes, void *stream);

/* ---- interpolation (replaces the CPU ops of tf_ops/tf_interpolate.cpp) --- */

/* threenn_cpu(b,n,m,xyz1,xyz2,dists,indices)  tf_interpolate.cpp:213-243.
 * xyz1 (b,n,3) unknown, xyz2 (b,m,3) known, m >= 3 -> dist (b,n,3) squared L2
 * ascending (computed in float64 like the reference's KD-tree), idx (b,n,3);
 * ties -> lowest index. */
int pn2_three_nn(int b, int n, int m, const float *xyz1, const float *xyz2,
                 float *dist, int *idx, void *stream);
/* pn2_three_nn with the QUERY rows ld1 floats apart (see pn2_fps_nested_ld) */
int pn2_three_nn_ld(int b, int n, int m, const float *xyz1, int ld1, const float *xyz2,
                    float *dist, int *idx, void *stream);

/* threeinterpolate_cpu(b,m,c,n,points,idx,weight,out)  tf_interpolate.cpp:307-330 */
int pn2_three_interpolate(int b, int m, int c, int n, const float *points,
                          const int *idx, const float *weight, float *out,
                          void *stream);

/* threeinterpolate_grad_cpu(b,n,c,m,grad_out,idx,weight,grad_points)
 * tf_interpolate.cpp:397-421.  grad_points (b,m,c) zeroed first. */
int pn2_three_interpolate_grad(int b, int n, int c, int m, const float *grad_out,
                               const int *idx, const float *weight,
                               float *grad_points, void *stream);

/* The same gradient with caller-provided scratch: large levels build a per-source-point list of (query, weight)
 * with 3*n integer atomics per cloud and then GATHER each grad_points row (no float atomics: 690 -> ~60 us on the
 * b=16, n=8192, m=1024, c=128 level of the training step); small levels, c % 4 != 0 or workspace == NULL run
 * pn2_three_interpolate_grad.  `workspace`: 4-byte aligned device scratch of at least
 * pn2_three_interpolate_grad_workspace_bytes(b, n, m) bytes.  Summation order varies from run to run. */
size_t pn2_three_interpolate_grad_workspace_bytes(int b, int n, int m);
int pn2_three_interpolate_grad_ws(int b, int n, int c, int m, const float *grad_out, const int *idx,
                                  const float *weight, float *grad_points, void *workspace,
                                  size_t workspace_bytes, void *stream);

/* The list of the two *_grad_ws calls above as an object of its own.  It depends on (idx, weight) only -- geometry, not
 * weights or activations -- so a training step builds it AHEAD (with the FPS / ball query / three_nn of the batch, beside the
 * previous step's dense work) and its backward pass only gathers:
 *   out[b, idx[b,e], :] = sum over the entries e with that idx of  w[b,e] * rows_in[b, e / div, 0:c]      (e < nent)
 *   groupPointGradLauncher      (tf_grouping.cu:155-162):   nent = m*nsample, div = 1, nsrc = n, weight_kind 0 (w = 1)
 *   threeinterpolate_grad_cpu   (tf_interpolate.cpp:397-421): nent = 3*n, div = 3, nsrc = m, weight_kind 1 (weight (b,n,3))
 *     or 2: `weight` holds three_nn's squared distances (b,n,3) and w is the inverse-distance weight of
 *     util/pointnet_util.py:300-303, formed with the float expressions of pn2_fp_interp_concat.
 * idx (b,nent) int32 in [0,nsrc).  plan: 4-byte aligned, pn2_scatter_plan_bytes(b,nent,nsrc) bytes, opaque, position
 * independent (may be copied).  apply: rows_in rows are `in_stride` floats apart (>= c: a column slice of a wider gradient
 * is read in place), c % 4 == 0, c <= 1024, out (b,nsrc,c) 16-byte aligned, overwritten (no zero fill needed).  The order
 * of a list (= the fp32 summation order) is fixed by the build. */
size_t pn2_scatter_plan_bytes(int b, int nent, int nsrc);
/* pn2_scatter_plan_build for up to 8 plans of one batch in ONE memset + three launches (a training step builds seven beside the
 * previous step's dense work): plan i = the pn2_scatter_plan_bytes(b, nent[i], nsrc[i]) bytes at buffer + offset[i] (offsets
 * ascending, 16-byte aligned, non-overlapping, inside buffer_bytes), each a plan pn2_scatter_plan_apply takes. */
int pn2_scatter_plan_build_multi(int nplans, int b, const int *nent, const int *div, const int *nsrc, const int *const *idx,
                                 const float *const *weight, const int *weight_kind, void *buffer, const size_t *offset,
                                 size_t buffer_bytes, void *stream);
int pn2_scatter_plan_build(int b, int nent, int div, int nsrc, const int *idx, const float *weight, int weight_kind,
                           void *plan, size_t plan_bytes, void *stream);
int pn2_scatter_plan_apply(int b, int nent, int div, int c, int nsrc, const float *rows_in, int in_stride,
                           const void *plan, size_t plan_bytes, float *out, void *stream);

/* pn2_scatter_plan_apply for nplans (<= 4) plans of one batch over the SAME nsrc source points in ONE launch (the scales of a
 * multi-scale SA module): plan i gathers rows_in[i] (rows in_stride[i] >= c[i] floats apart) into columns [ocol[i], ocol[i] + c[i])
 * of the shared out (b,nsrc,out_stride).  Every element of those column blocks is written (no zero fill needed), in the plan's
 * summation order: each block holds the bits pn2_scatter_plan_apply writes for that plan alone; columns outside every block are
 * left alone.  nent / div / c / ocol / rows_in / in_stride / plan / plan_bytes: host arrays read at call time.  c[i] % 4 == 0,
 * c[i] <= 1024; ocol[i] % 4 == 0, blocks ascending and disjoint; out_stride % 4 == 0, out 16-byte aligned (PN2_EUNSUP /
 * PN2_EINVAL otherwise, as pn2_scatter_plan_apply). */
int pn2_scatter_plan_apply_multi(int nplans, int b, int nsrc, int out_stride, const int *nent, const int *div, const int *c,
                                 const int *ocol, const float *const *rows_in, const int *in_stride, const void *const *plan,
                                 const size_t *plan_bytes, float *out, void *stream);

/* n (<= 48) independent device-to-device copies in ONE launch: dst[i][0..bytes[i]) = src[i][0..bytes[i]); the three arrays
 * are host arrays read at call time; regions must not overlap.  Training-step plumbing: a batch's geometry tensors (mixed
 * int32 / float32 / byte buffers) into the static buffers the captured step reads. */
int pn2_multi_copy(int n, const void *const *srcs, void *const *dsts, const unsigned long long *bytes, void *stream);
/* pn2_multi_copy + nfill (<= 4) scalar stores of 4 or 8 bytes in the same launch: *fill_dsts[i] = low fill_bytes[i] bytes of
 * fill_vals[i] (host arrays; the values travel in the launch arguments).  A captured training step's per-step scalars (Adam's
 * bias-corrected rate, the dropout step) ride with its input copy. */
int pn2_multi_copy_fill(int n, const void *const *srcs, void *const *dsts, const unsigned long long *bytes, int nfill,
                        void *const *fill_dsts, const unsigned long long *fill_vals, const int *fill_bytes, void *stream);

/* ---- fused layer kernels (new: no reference kernel; they replace the TF
 *      sub-graphs of util/pointnet_util.py:44-54,150-170 and :300-325) ------- */

/* One dense layer of the shared MLP with the BatchNorm folded in (inference):
 *   y = relu?( x @ W + bias )           x (rows,cin)  W (cin,cout)  y (rows,cout)
 * optionally followed by a max over each consecutive group of `pool` rows
 * (pool = nsample reproduces tf.reduce_max over K, pointnet_util.py:167-170;
 * pool <= 1 = no pooling; otherwise pool must be 32 or a multiple of 32 ... see
 * DESIGN.md).  y is (rows/pool, cout) when pooling.  fp32 MFMA, exact-f32
 * products, fp32 accumulation. */
int pn2_linear(int rows, int cin, int cout, const float *x, const float *w,
               const float *bias, int relu, int pool, float *y, void *stream);

/* Weight gradient of that layer for the training path: dw (cin,cout) = x^T (cin,rows) . dy (rows,cout), overwritten.
 * (The reduction over all B*M*K rows that TF / hipBLASLt run as a tall-skinny GEMM.)  fp32 MFMA, partial tiles
 * merged with fp32 atomics: the summation order varies from run to run like the reference's atomicAdd gradients. */
int pn2_linear_wgrad(int rows, int cin, int cout, const float *x, const float *dy, float *dw, void *stream);
/* dw += x^T . dy (no zero fill: the caller owns the initial value, e.g. a gradient arena zero-filled once per step). */
int pn2_linear_wgrad_accumulate(int rows, int cin, int cout, const float *x, const float *dy, float *dw, void *stream);

/* Training-mode batch normalisation + ReLU of a dense layer's output y (rows,c), channels last
 * (util/tf_util.py:555-581 batch_norm_template -> tf.contrib.layers.batch_norm, applied by conv2d / conv1d /
 * fully_connected at tf_util.py:186-204 and followed by tf.nn.relu):
 *   mean, var = per-channel batch moments over all rows (biased var; fp64 accumulation)
 *   z = relu?( gamma * (y - mean) / sqrt(var + eps) + beta )
 *   running_mean = decay*running_mean + (1-decay)*(mean + bias),  running_var likewise with the UNBIASED batch variance
 * `bias` (nullable, (c)) is the layer bias the caller folded away: a per-channel constant in front of BN only moves
 * the mean, so it enters the moving average and nothing else.  running_mean / running_var may both be NULL.
 * pool > 1 fuses the SA layer's max over each group of `pool` consecutive rows (tf.reduce_max over the K neighbours,
 * pointnet_util.py:167-170): z is then (rows/pool, c) and `ties` (rows/pool, c) receives the number of rows that
 * attain the maximum (the gradient is shared equally among them, as tf / torch do); the (rows,c) activation is never
 * written.  pool <= 1: z is (rows,c), ties unused (NULL).
 * save_mean / save_invstd (c) are kept for pn2_bn_relu_backward.  `workspace`: 8-byte aligned device scratch of at
 * least pn2_bn_workspace_bytes(c) bytes (fp64 per-channel accumulators, contents irrelevant on entry).
 * c <= 1024; c % 4 != 0 needs c <= 256. */
size_t pn2_bn_workspace_bytes(int c);
int pn2_bn_relu_forward(long long rows, int c, const float *y, const float *gamma, const float *beta,
                        const float *bias, float eps, float decay, int relu, int pool, float *running_mean,
                        float *running_var, void *workspace, size_t workspace_bytes, float *save_mean,
                        float *save_invstd, float *z, float *ties, void *stream);
/* Its gradient (what tf.gradients derives for the ops above): with g = dz * [z > 0] (relu; behind the fused max
 * pool dz (rows/pool,c) first goes to the rows that attain zmax, divided by `ties`) and xhat = (y - mean) * invstd,
 *   dbeta = sum_r g,  dgamma = sum_r g*xhat,  dy = gamma*invstd * (g - dbeta/rows - xhat * dgamma/rows).
 * zmax / ties: the forward's z / ties when pool > 1 (else NULL).  dy (rows,c) may alias dz when pool <= 1.  The ReLU
 * mask and the pooled maxima are recomputed from y with the forward's own float expressions. */
int pn2_bn_relu_backward(long long rows, int c, const float *dz, const float *y, const float *gamma,
                         const float *beta, const float *save_mean, const float *save_invstd, int relu,
                         int pool, const float *zmax, const float *ties, void *workspace,
                         size_t workspace_bytes, float *dy, float *dgamma, float *dbeta, void *stream);
/* The state of a batch-norm workspace when a call arrives = the `stats_mode` argument (an int) of pn2_bn_relu_forward_mode,
 * pn2_bn_relu_forward_pool and pn2_bn_relu_backward_mode; any other value is PN2_EINVAL.  The two calls above are UNCLEARED.
 *   UNCLEARED  contents irrelevant: the call zeroes the workspace itself.
 *   ZEROED     the caller zeroed it: one fill of an arena holding the scratch of every layer of a training step replaces one
 *              memset per call (88 per step for the semantic.json model).
 *   SUMMED     zeroed by the caller, and a producer has added its sums (forward: y, y*y; backward, pool <= 1: g, g*xhat) to all
 *              slot copies: the call folds them and skips its reduction pass.  Left by pn2_linear_bn_stats, pn2_linear_bn_stats_xf,
 *              pn2_linear_dgrad_bn_grad_stats, pn2_linear_dgrad_gx with y_below, and the entry points below with finish 0.
 *   FOLDED     the sums are there and the producer's last workgroup has folded them: only the normalisation pass is left.  Left
 *              by pn2_linear_bn_stats_fin, pn2_sa_first_layer_bn, pn2_*_hoist_rows*_bn with finish 1 and by pn2_linear_dgrad_fin,
 *              pn2_linear_bwd_fused with finish_below 1. */
enum { PN2_BN_WS_UNCLEARED = 0, PN2_BN_WS_ZEROED = 1, PN2_BN_WS_SUMMED = 2, PN2_BN_WS_FOLDED = 3 };
/* conv2d -> batch_norm of the training path (util/tf_util.py:186-204) without the statistics pass over y:
 * pn2_linear_bn_stats computes y (rows,cout) = x (rows,cin) . w (cin,cout) (no bias, no activation; cout % 32 == 0)
 * and adds the column sums of y and y*y to `bn_workspace` (pn2_bn_workspace_bytes(cout) bytes, ZEROED by the caller)
 * from the GEMM's accumulators, which leaves it PN2_BN_WS_SUMMED for pn2_bn_relu_forward_mode / _pool. */
int pn2_linear_bn_stats(int rows, int cin, int cout, const float *x, const float *w, float *y,
                        void *bn_workspace, size_t workspace_bytes, void *stream);

/* Fused set-abstraction MLP (pointnet_util.py:43-54 + :150-170, inference BN
 * folded): for every (b, j) group gathers nsample neighbours by idx, builds
 * [xyz[idx]-new_xyz | points[idx]] (xyz first, pointnet_util.py:52-54), runs up
 * to 3 dense layers (+bias, ReLU) and max-pools over the neighbours without the
 * grouped tensor ever reaching HBM.
 *   xyz (b,n,3)  new_xyz (b,m,3)  points (b,n,c) or NULL (c = 0)  idx (b,m,nsample)
 *   w[l] (cin_l, widths[l]) row-major with cin_0 = 3 + c;  bias[l] (widths[l])
 *   out (b,m,widths[nlayers-1])
 * Constraints: nsample 16, 32, 64, 128 or 256 (32 is the native tile; 16 needs b*m even), 1 <= nlayers <= 3,
 * widths multiples of 32, <= 128 and a supported layer pattern (returns PN2_EUNSUP otherwise: callers fall back
 * to pn2_group_point + pn2_linear). */
int pn2_sa_mlp_max_fused(int b, int n, int m, int nsample, int c, const float *xyz,
                         const float *new_xyz, const float *points, const int *idx,
                         int nlayers, const int *widths, const float *const *w,
                         const float *const *bias, float *out, void *stream);
/* pn2_sa_mlp_max_fused with the rows of xyz / points ld_xyz / ld_points floats apart (see pn2_fps_nested_ld); a strided
 * `points` needs the un-vectorised feature path (c % 8 != 0), else PN2_EUNSUP. */
int pn2_sa_mlp_max_fused_ld(int b, int n, int m, int nsample, int c, const float *xyz, int ld_xyz,
                            const float *new_xyz, const float *points, int ld_points, const int *idx,
                            int nlayers, const int *widths, const float *const *w,
                            const float *const *bias, float *out, void *stream);

/* bf16 variant of pn2_sa_mlp_max_fused (BASELINE configs[4]: large-scene inference, nsample 64): points is
 * (b,n,c) bfloat16, weights/biases are fp32 and are rounded to bf16 (RNE) by the kernel, products exact,
 * fp32 accumulation, hidden activations bf16(relu(acc+bias)), out (b,m,widths[last]) fp32 -- the precision
 * contract is spelled out in csrc/pn2_sa_fused_bf16.hip and restated by oracle.mlp_max_bf16.
 * Constraints: nsample 32 or 64, c % 16 == 0, points 16-byte aligned, widths multiples of 32 <= 128, a
 * supported layer pattern ([128], [128,128], [64,128], [64,64,128], [128,128,128]); PN2_EUNSUP otherwise. */
int pn2_sa_mlp_max_fused_bf16(int b, int n, int m, int nsample, int c, const float *xyz,
                              const float *new_xyz, const void *points_bf16, const int *idx,
                              int nlayers, const int *widths, const float *const *w,
                              const float *const *bias, float *out, void *stream);

/* Same gather + MLP chain without the max over the neighbours: out (b,m,nsample,widths[last]),
 * ReLU applied.  Feeds a wider last layer that runs on pn2_linear with pool = nsample.
 * Supported: nsample == 32, widths [128] or [128,128]; PN2_EUNSUP otherwise. */
int pn2_sa_mlp_rows_fused(int b, int n, int m, int nsample, int c, const float *xyz,
                          const float *new_xyz, const float *points, const int *idx,
                          int nlayers, const int *widths, const float *const *w,
                          const float *const *bias, float *out, void *stream);

/* Fused feature-propagation front end (pointnet_util.py:300-311):
 *   weight = (1/max(dist,1e-10)) / sum(1/max(dist,1e-10));
 *   out[b,j,:] = [ sum_i weight_i * points2[b,idx_i,:]  |  points1[b,j,:] ]
 * i.e. three_interpolate + concat (interpolated FIRST) in one pass.
 *   dist,idx (b,n,3)  points2 (b,m,c2)  points1 (b,n,c1) or NULL -> out (b,n,out_stride)
 * out_stride >= c2+c1 (0 = c2+c1): row stride of `out`; pad columns are zero-filled so that the
 * consumer can use 16-byte loads (e.g. 131 -> 136). */
int pn2_fp_interp_concat(int b, int n, int m, int c1, int c2, const float *dist,
                         const int *idx, const float *points1, const float *points2,
                         float *out, int out_stride, void *stream);

/* Dense-row MLP chain (pointnet_util.py:312-325, inference BN folded): up to 2 layers
 *   y = relu(relu(x @ W0 + b0) @ W1 + b1)      x (rows,cin)  W_l (cin_l, widths[l])
 * with all weights resident in LDS and the hidden activation kept in registers; pool = 32 adds a
 * max over each consecutive group of 32 rows (y is (rows/32, w_last)), pool = 0 keeps all rows.
 * widths multiples of 32, <= 128; PN2_EUNSUP when the configuration does not fit (callers fall
 * back to pn2_linear). */
int pn2_mlp_chain(int rows, int cin, const float *x, int nlayers, const int *widths,
                  const float *const *w, const float *const *bias, int pool, float *y,
                  void *stream);

/* Wide dense-row MLP chain for the coarse levels (SA3 tail, SA4, FP2, FP3: pointnet_util.py:150-170 and :312-325,
 * inference BN folded): up to 3 layers with widths in {128, 256, 512},
 *   y = act(...relu(relu(x @ W0 + b0) @ W1 + b1)...)     x (rows, x_stride >= cin)   W_l (cin_l, widths[l]) row-major
 * one workgroup per 32-row tile through all layers (activations in LDS, weights streamed from L2); relu_last selects the
 * activation of the last layer; pool = 32: max over each group of 32 consecutive rows, y (rows/32, w_last); pool = 0:
 * y (rows, w_last).  w, bias, y 16-byte aligned; W0 must hold ((cin + 7) & ~7) rows (zero rows behind the cin real ones:
 * the kernel contracts in groups of 8).  PN2_EUNSUP when the configuration does not fit (callers fall back to pn2_linear
 * per layer). */
int pn2_mlp_wide(int rows, int cin, int x_stride, const float *x, int nlayers, const int *widths,
                 const float *const *w, const float *const *bias, int relu_last, int pool, float *y, void *stream);
/* The same chain behind the SA front end (pointnet_util.py:39-54: group_point, centre, concat [xyz | features]) for
 * nsample = 32: rows are gathered through idx (b,m,32) straight into the first layer's operand tile.  W0's rows in the
 * order the tile is built in: [features (c rows) | x y z (3 rows) | zero rows up to a multiple of 8] (the reference's
 * variable is [xyz | features]: the caller rotates it once).  pool != 0: max over the 32 neighbours, y (b,m,w_last);
 * else (b,m,32,w_last). */
int pn2_sa_mlp_wide(int b, int n, int m, int nsample, int c, const float *xyz, const float *new_xyz,
                    const float *points, const int *idx, int nlayers, const int *widths, const float *const *w,
                    const float *const *bias, int pool, float *y, void *stream);
/* ... and behind the FP front end (pointnet_util.py:300-311), i.e. pn2_fp_interp_concat + pn2_mlp_wide in one kernel:
 *   x[b,j,:] = [ three_interpolate(points2, idx, w(dist))[b,j,:] | points1[b,j,:] ]   (never stored)
 * dist,idx (b,n,3)  points2 (b,m,c2)  points1 (b,n,c1) or NULL; n % 32 == 0, c1 % 4 == 0, c2 % 4 == 0; W0 holds
 * ((c2 + c1 + 7) & ~7) rows, interpolated channels first  ->  y (b*n, w_last), ReLU after every layer. */
int pn2_fp_mlp_wide(int b, int n, int m, int c1, int c2, const float *dist, const int *idx, const float *points1,
                    const float *points2, int nlayers, const int *widths, const float *const *w,
                    const float *const *bias, float *y, void *stream);

/* Fused feature-propagation block (pointnet_util.py:300-325, inference BN folded):
 *   x[b,j,:] = [ three_interpolate(points2, idx, w(dist))[b,j,:] | points1[b,j,:] ]   (never stored)
 *   y = relu(relu(x @ W0 + b0) @ W1 + b1)                                            (nlayers 1 or 2)
 * i.e. pn2_fp_interp_concat + pn2_mlp_chain in one kernel: the interpolated rows go from L2 straight
 * into the MFMA operands.  dist,idx (b,n,3)  points2 (b,m,c2)  points1 (b,n,c1) or NULL
 * w[0] (>= c2+c1 rows, widths[0]), interpolated channels first  ->  y (b*n, widths[nlayers-1]).
 * Constraints: c2 % 8 == 0, widths multiples of 32 and <= 128; PN2_EUNSUP otherwise. */
int pn2_fp_mlp_fused(int b, int n, int m, int c1, int c2, const float *dist, const int *idx,
                     const float *points1, const float *points2, int nlayers, const int *widths,
                     const float *const *w, const float *const *bias, float *y, void *stream);

/* ---- post-processing next to the path ----------------------- */

/* interpolate_label_with_color_cpu(num_sparse_points, num_dense_points, sparse_points, sparse_labels,
 * dense_points, dense_labels, dense_colors, knn)  tf_interpolate.cpp:71-115 (CPU + Open3D KD-tree in the
 * reference).  sparse_points (ns,3), sparse_labels (ns), dense_points (nd,3) -> dense_labels (nd) int32,
 * dense_colors (nd,3) uint8: majority label among the min(knn, ns) nearest sparse points (exact, float64
 * squared L2, ascending, ties -> lowest index; vote and colour table of :45-47,96-113).  ns == 0 gives
 * label -1 / colour 0; labels outside [0,9) get colour 0 (both undefined behaviour in the reference).
 * `workspace`: 256-byte aligned device scratch of at least pn2_interpolate_label_workspace_bytes(ns)
 * bytes (uniform grid over the sparse points).  knn <= 16 (PN2_EUNSUP above). */
size_t pn2_interpolate_label_workspace_bytes(int num_sparse_points);
int pn2_interpolate_label_with_color(int num_sparse_points, int num_dense_points,
                                     const float *sparse_points, const int *sparse_labels,
                                     const float *dense_points, int *dense_labels,
                                     uint8_t *dense_colors, int knn, void *workspace,
                                     size_t workspace_bytes, void *stream);

/* ---- training step ----------------------------------------------------------------- */

/* Data gradient of a dense layer: dx (rows,cin) = dy (rows,cout) . W^T, W (cin,cout) row-major as the forward pass holds
 * it; any cin / cout (tf.gradients of tf.nn.conv2d, util/tf_util.py:181-186). */
int pn2_linear_dgrad(int rows, int cin, int cout, const float *dy, const float *w, float *dx, void *stream);
/* The same when dx IS the gradient reaching the batch norm (+ReLU) of the layer below (the layer whose output is this
 * layer's input, consumed by nothing else): y_below (rows,cin) = that layer's pre-normalisation output, gamma / beta /
 * save_mean / save_invstd its parameters and saved batch moments, relu its activation flag.  While the accumulator tiles of
 * dx are at hand the kernel adds sum g and sum g*xhat per channel (g = dx * [ReLU mask], xhat = (y-mean)*invstd) to that
 * layer's ZEROED batch-norm workspace (pn2_bn_workspace_bytes(cin) bytes), which leaves it PN2_BN_WS_SUMMED:
 * pn2_bn_relu_backward_mode then skips its reduction pass over (dz, y).  Same results up to fp64 summation order.
 * PN2_EUNSUP for cout <= 16 (streaming kernel): use pn2_linear_dgrad + pn2_bn_relu_backward.
 * (tf.gradients through tf_util.py:186-204: conv2d -> batch_norm -> relu.) */
int pn2_linear_dgrad_bn_grad_stats(int rows, int cin, int cout, const float *dy, const float *w, float *dx,
                                   const float *y_below, const float *gamma, const float *beta, const float *save_mean,
                                   const float *save_invstd, int relu, void *bn_workspace, size_t workspace_bytes,
                                   void *stream);

/* model.get_loss  model.py:152-161: weighted sparse softmax cross-entropy, reduction SUM_BY_NONZERO_WEIGHTS.
 * logits (rows,num_class) f32, labels (rows) int32 (label64 = 0) or int64 (label64 = 1), weights (rows) f32 ->
 * *loss (device f32) = sum_r w_r*ce_r / max(1, #{w_r != 0}).  lse (rows) f32 and acc (2 doubles, zeroed by the callee)
 * carry the forward's results to the backward.  num_class <= 64.
 * A row whose label lies outside [0, num_class) behaves as a row of weight 0: it adds nothing to the sum, is not counted
 * in #{w_r != 0}, and gets a zero gradient row from the backward (its lse is still written).  An int64 label is compared at
 * 64 bits: 2^32 + 3 is out of range although its low word is a class.  pn2_confusion_update sets the same rows aside.
 * PN2_EINVAL: rows <= 0 or num_class <= 0; PN2_EUNSUP: num_class > 64; PN2_ENULL: a NULL pointer other than gout. */
int pn2_weighted_ce_forward(int rows, int num_class, const float *logits, const void *labels, int label64,
                            const float *weights, float *lse, double *acc, float *loss, void *stream);
/* d loss / d logits = gout * w_r / nz * (softmax_r - onehot_r), a row of zeros where the label is out of range;
 * gout: device scalar (upstream gradient) or NULL (= 1). */
int pn2_weighted_ce_backward(int rows, int num_class, const float *logits, const void *labels, int label64,
                             const float *weights, const float *lse, const double *acc, const float *gout,
                             float *dlogits, void *stream);

/* The per-batch metrics of the reference's train_one_epoch / eval_one_epoch (train.py:199-331, util/metric.py) on the
 * device.  logits (rows,num_class) f32 contiguous, labels (rows) int32 (label64 = 0) or int64 (label64 = 1).  Per row the
 * argmax with np.argmax semantics (first maximal index wins ties, a NaN counts as the maximum and the first NaN wins, +-inf
 * compare normally); every output is optional:
 *   pred (rows) int32         <- the argmax;
 *   confusion (num_class^2)   += 1 at [label * num_class + pred] (accumulates across calls, never zeroed here); a label
 *                                outside [0, num_class) is left out and counted in *invalid;
 *   loss_acc (2 doubles)      += {*loss, 1} (loss: device f32 scalar; both or neither).
 * PN2_EINVAL: rows <= 0, num_class <= 0, no output requested, or only one of loss / loss_acc; PN2_EUNSUP: num_class > 64;
 * PN2_ENULL: logits or labels NULL.  No host synchronisation, no allocation: capturable into a graph. */
int pn2_confusion_update(int rows, int num_class, const float *logits, const void *labels, int label64, int *pred,
                         long long *confusion, long long *invalid, const float *loss, double *loss_acc, void *stream);

/* ConfusionMatrix.increment_from_list (util/metric.py) on the device: confusion[gt*C + pd] += 1 for every pair with both
 * labels in [0, C); other pairs are dropped (sklearn's confusion_matrix(labels=range(C))) and, when dropped != NULL,
 * counted there.  gt / pd: n labels each, int32 (label64 == 0) or int64 (label64 != 0: values beyond int32 must not wrap).
 * confusion (C*C) and *dropped accumulate across calls and are never zeroed here.  Exact, independent of arrival order: each
 * workgroup counts into a private uint32 histogram and adds its non-zero bins once, which bounds n at 2^39 pairs per call.
 * PN2_EINVAL: n <= 0, n > 2^39 or num_class <= 0; PN2_EUNSUP: num_class > 64; PN2_ENULL: gt, pd or confusion NULL.
 * No host synchronisation, no allocation: capturable into a graph. */
int pn2_label_confusion(long long n, int num_class, const void *gt, const void *pd, int label64,
                        long long *confusion, long long *dropped, void *stream);

/* tf_util.dropout  util/tf_util.py:646-665 (tf.nn.dropout): y = x / keep_prob where kept, else 0; mask (n bytes) for the
 * backward.  state: device int64[2] = {seed, step}; the draw is a pure function of (seed, step, element index), so a
 * captured graph can be replayed while the caller advances `step` in device memory.  keep_prob = 1 keeps every element
 * whatever it draws.  PN2_EINVAL: n <= 0, or keep_prob not in (0, 1] (NaN included). */
int pn2_dropout(long long n, const float *x, float keep_prob, const long long *state, float *y,
                unsigned char *mask, void *stream);
int pn2_dropout_grad(long long n, const float *dy, const unsigned char *mask, float keep_prob, float *dx,
                     void *stream);

/* Backward of bias + ReLU on a layer WITHOUT batch norm (util/tf_util.py:186-204 with bn=False, tf.nn.relu's ReluGrad):
 * dx[i] = z[i] > 0 ? dz[i] : 0 over n elements, z = the layer's OUTPUT; dx may alias dz. */
int pn2_relu_grad(long long n, const float *z, const float *dz, float *dx, void *stream);

/* tf.train.AdamOptimizer.apply_gradients  train.py:381-388, one launch over flat fp32 buffers of n elements:
 * m <- b1 m + (1-b1) g;  v <- b2 v + (1-b2) g^2;  p <- p - lr_t * m / (sqrt(v) + eps), g = grads * grad_scale.
 * hyper: DEVICE float[5] = {lr_t, beta1, beta2, epsilon, grad_scale}, lr_t = lr*sqrt(1-beta2^t)/(1-beta1^t). */
int pn2_adam_step(long long n, float *params, const float *grads, float *m, float *v, const float *hyper,
                  void *stream);

/* tf.train.MomentumOptimizer(lr, momentum).apply_gradients, use_nesterov = False (train.py:380-383), one launch over flat
 * fp32 buffers of n elements:  g' = grads[i] * grad_scale;  accum[i] = momentum * accum[i] + g';  params[i] -= lr * accum[i]
 * hyper: DEVICE float[3] = {lr, momentum, grad_scale}  (lr first: it is the per-step slot a captured step rewrites) */
int pn2_momentum_step(long long n, float *params, const float *grads, float *accum, const float *hyper, void *stream);

/* sample_and_group's tail for layers too wide for the fused kernel (util/pointnet_util.py:39-54: group_point(xyz) -
 * tile(new_xyz), group_point(points), concat [xyz | points]) in one pass: out (b,m,nsample,3+c) with
 * out[..., :3] = xyz[idx] - new_xyz and out[..., 3:] = points[idx] (c may be 0, then points may be NULL). */
int pn2_sa_group_concat(int b, int n, int m, int nsample, int c, const float *xyz, const float *new_xyz,
                        const float *points, const int *idx, float *out, void *stream);

/* ---- the step before the path: scene sampler + voxel down-sampling ---------------- */

/* SemanticFileData._extract_z_box  dataset/semantic_dataset.py:123-163, for b centre points at once.
 * points (n,3) float64 sorted by x (as __init__ leaves them, :84-88); centers (b,3) float64; half_x/half_y =
 * box_size/2; scene_z_size = max z - min z of the scene (:132).  out_idx (b,cap) = scene indices of every column in
 * scene order, out_cnt (b) = their number (may exceed cap: then only the first cap indices were written). */
int pn2_scene_extract_z_box(int n, const double *points, int b, const double *centers, double half_x,
                            double half_y, double scene_z_size, int cap, int *out_idx, int *out_cnt,
                            void *stream);

/* _get_fix_sized_sample_mask + gathers + _center_box  semantic_dataset.py:90-121,165-186.  The reference's random
 * draw enters as `mask` (b,cap) bytes: for a column with cnt > npts its first cnt bytes are the shuffled boolean
 * sample mask (exactly npts non-zero); columns with cnt <= npts repeat their indices (i mod cnt) and ignore it.
 * labels (n) int32 / colors (n,3) float64 may be NULL (zeros out).  Outputs: out_sel (b,npts) scene indices,
 * out_centered (b,npts,3) float32 = float64 (p - shift) cast, out_raw (b,npts,3) float64, out_labels (b,npts),
 * out_colors (b,npts,3) float32 (the last three optional).  status (b): 0 ok, 1 empty column, 2 cnt > cap,
 * 3 mask does not select exactly npts points. */
int pn2_scene_sample(int b, int npts, int cap, const double *points, const int *labels, const double *colors,
                     const int *idx, const int *cnt, const unsigned char *mask, double half_x, double half_y,
                     int *out_sel, float *out_centered, double *out_raw, int *out_labels, float *out_colors,
                     int *status, void *stream);

/* down_sample  downsample.py:46-67: Open3D (IntelVCL/Open3D @33e46f7) voxel_down_sample_and_trace with
 * min_bound = min(points) - voxel_size/2 + np.bincount(labels).argmax() per voxel.  points/colors (n,3) float64,
 * labels (n) int32 in [0,64) or NULL.  Outputs sized for n voxels; *out_count (device) = number of voxels, sorted by
 * (ix,iy,iz) (Open3D's own order is unspecified).  status (device): 0 ok, 1 voxel index needs more than 21 bits,
 * 2 label outside [0,64), 3 a NaN or +-inf coordinate (outranks 1; a bad label in the same cloud may leave 2 instead).
 * With a non-zero status the outputs are written inside their n rows but hold nothing of use.  out_colors and
 * out_labels may be NULL.  n <= 0 is PN2_EINVAL: a caller with nothing to down-sample does not call.
 * workspace: 256-byte aligned, pn2_voxel_downsample_workspace_bytes(n) bytes. */
size_t pn2_voxel_downsample_workspace_bytes(int n);
int pn2_voxel_downsample(int n, const double *points, const double *colors, const int *labels, double voxel_size,
                         double *out_points, double *out_colors, int *out_labels, int *out_count, int *status,
                         void *workspace, size_t workspace_bytes, void *stream);

/* SemanticDataset.sample_batch_in_all_files  dataset/semantic_dataset.py:214-343 + util/provider.py rotate_*point_cloud,
 * on a device-resident multi-scene store, in four launches (csrc/pn2_dataset.hip).
 * Store: points (total,3) float64, every scene x-sorted in its segment [scene_offsets[k], scene_offsets[k+1]);
 * colors (total,3) float32 or NULL (zeros), labels (total) uint8 or NULL (zeros); scene_cdf (num_scenes) float64 =
 * cumsum(p) / its last entry; scene_z_size (num_scenes) = max z - min z; label_weights (num_label_weights) float32
 * (weight of a label >= num_label_weights: 0).  max_chunks >= ceil(largest scene / 1024).
 * Draws: draw_scene == NULL -> device random numbers from seed and *counter (device int64, advanced by one per call by the
 * last launch, so a captured call replays into fresh batches); else replay: draw_scene / draw_center (b) int32 (centre
 * relative to its scene), draw_mask (b,mask_cap) bytes = the reference's shuffled boolean mask for columns larger than
 * npts, draw_rot (b,3) float64 = angle, cos, sin (required with augment).
 * Workspace: 256-byte aligned, pn2_dataset_workspace_size(b, max_chunks) bytes, zero before the first call (calls keep it
 * zero; one call at a time per workspace).
 * Outputs: out_info (b,8) int32 = scene, centre, column count, slab lo, slab hi, key bin, candidates needed, status
 * (0 ok, 1 empty column or bad draw, 2 column wider than mask_cap, 3 mask does not select npts, 4 candidate list full,
 * 5 slab longer than max_chunks: such a sample is zero-filled); out_finfo (b,3) float64 = angle, cos, sin;
 * out_sel (b,npts) int32 store indices of the chosen points in scene order, repeated i mod count when count <= npts (-1
 * for a rejected sample);
 * out_data (b,npts,6|3) float32 rows [xyz | rgb]; out_labels (b,npts) int32; out_weights (b,npts) float32. */
int pn2_dataset_workspace_size(int b, int max_chunks, unsigned long long *bytes);
int pn2_dataset_sample(int b, int npts, int num_scenes, int max_chunks, int use_color, int augment, const double *points,
                       const float *colors, const unsigned char *labels, const int *scene_offsets, const double *scene_cdf,
                       const double *scene_z_size, const float *label_weights, int num_label_weights, double half_x,
                       double half_y, unsigned long long seed, long long *counter, const int *draw_scene,
                       const int *draw_center, const unsigned char *draw_mask, int mask_cap, const double *draw_rot,
                       void *workspace, size_t workspace_bytes, int *out_info, double *out_finfo, int *out_sel,
                       float *out_data, int *out_labels, float *out_weights, void *stream);

/* One scene of that store built on the device (csrc/pn2_store.hip): SemanticFileData.__init__ dataset/semantic_dataset.py:84-88
 * (sort by x, gather) plus what SemanticDataset.__init__ (:214-290) takes from the sorted scene.  Inputs: points (n,3) float64,
 * colors (n,3) float64 or NULL, labels (n) int32 or NULL.  The rule:
 *   order      output row i is input row perm[i]; perm sorts by points[:, 0] ascending, ties broken by input index
 *              (np.argsort(x, kind="stable"); the reference's default argsort leaves the order of ties unspecified).  -0.0 and
 *              +0.0 compare equal, as in numpy: the key treats them as one value, the stored value keeps its sign.
 *   out_points (n,3) float64: the rows copied bit for bit.
 *   out_colors (n,3) float32: float64 -> float32 by one IEEE rounding (numpy astype(np.float32)).  colors == NULL: nothing is
 *              read or written for colours (out_colors may be NULL).
 *   out_labels (n) uint8: int32 -> uint8; labels == NULL writes zeros.  A label outside [0, 255] sets status 2.
 *   out_zrange (2) float64 = [min z, max z] of the scene, exact (scene_z_size is their one subtraction, left to the caller);
 *              among zeros -0.0 counts as the smaller, so the pair does not depend on the order of the rows.
 *   out_hist   (9) int64 = np.histogram(labels, range(10))[0]: labels 8 and 9 share the last bin, labels above 9 are valid
 *              but counted nowhere; labels == NULL: all n in bin 0.
 *   status     (1) int32: 0 ok; 1 a NaN or +-inf in x, y or z (the host path sorts NaN last and then mis-searches; this one
 *              refuses); 2 a label outside [0, 255]; both: 1.  With a non-zero status the other outputs are written inside
 *              their n rows like any others, but what they hold is not specified.
 *   out_perm   (n) int32 = perm, or NULL.
 * Every output may point into the middle of a larger store: nothing outside rows [0, n) of each is written.  No output may
 * overlap an input.  Pointers naturally aligned; workspace 256-byte aligned, pn2_scene_ingest_workspace_size(n) bytes (a
 * workspace sized for one n serves any n whose own size is not larger), no state kept between calls.
 * Four launches and a radix sort (hipcub, 64 key bits, stable); every reduction is in integers or ordered keys, so every
 * result is independent of the order in which workgroups arrive.  No host synchronisation.
 * PN2_EINVAL: n <= 0, workspace too small, a misaligned pointer; PN2_ENULL: points, out_points, out_labels, out_zrange,
 * out_hist, status or workspace NULL, or out_colors NULL while colors is not: refused before any launch. */
int pn2_scene_ingest_workspace_size(int n, unsigned long long *bytes);
int pn2_scene_ingest(int n, const double *points, const double *colors, const int *labels, double *out_points,
                     float *out_colors, unsigned char *out_labels, int *out_perm, double *out_zrange, long long *out_hist,
                     int *status, void *workspace, size_t workspace_bytes, void *stream);

/* pn2_fp_mlp_fused with the first layer's product with the INTERPOLATED channels hoisted out by linearity:
 * three_interpolate(points2) @ W1a == three_interpolate(points2 @ W1a) (pointnet_util.py:300-311 followed by the first conv
 * of :312-325), and z = points2 @ W1a has the m known rows per cloud instead of the n unknown ones.  z (b*m, widths[0])
 * replaces points2; w[0] = the c1 skip-link rows of the folded first-layer weight (c1 x widths[0]; NULL when c1 == 0),
 * w[1..] / bias[0..] as in pn2_fp_mlp_fused.  nlayers = 2 or 3 (all widths multiples of 32, <= 128, LDS-resident).
 * fp32 results differ from the un-hoisted order by rounding only (~1e-7 of the activation scale). */
int pn2_fp_mlp_fused_pre(int b, int n, int m, int c1, const float *dist, const int *idx, const float *points1,
                         const float *z, int nlayers, const int *widths, const float *const *w,
                         const float *const *bias, float *y, void *stream);
/* pn2_fp_mlp_fused_pre with the skip-link rows ld_points1 floats apart (see pn2_fps_nested_ld) */
int pn2_fp_mlp_fused_pre_ld(int b, int n, int m, int c1, const float *dist, const int *idx, const float *points1,
                            int ld_points1, const float *z, int nlayers, const int *widths, const float *const *w,
                            const float *const *bias, float *y, void *stream);

/* pn2_fp_mlp_fused_pre with the kernel SCHEDULE named by the caller (stateless door for parity tests / A-B timing):
 * 0 = lockstep kernel (8 waves: gather, MFMA layers, store), 1 = software-pipelined kernel (one wave per SIMD builds the next
 * tile's first-layer accumulator between the MFMA groups of the current tile; three 128-wide layers, c1 <= 8, else
 * PN2_EUNSUP).  Same bits either way; pn2_fp_mlp_fused_pre picks 1 where it applies. */
int pn2_fp_mlp_fused_pre_schedule(int b, int n, int m, int c1, const float *dist, const int *idx, const float *points1,
                                  const float *z, int nlayers, const int *widths, const float *const *w,
                                  const float *const *bias, float *y, int schedule, void *stream);

/* Row packing of the pooled nsample = 32 set-abstraction kernels (pn2_sa_mlp_max_fused, _ld, pn2_sa_mlp_fused_pre with
 * pool; pn2_sa_mlp_wide and pn2_sa_mlp_wide_pre with pool and an idx that is 16-byte aligned): the ball query pads a short
 * row with copies of its first hit; the kernels find the live prefix of every index row (the smallest s in {8, 16, 32} with
 * idx[j] == idx[0] for all j >= s, read from idx itself) and put four centres with s = 8 or two with s = 16 into one 32-row
 * matrix tile.  Same bits as without it for ANY index table.  One switch for all of them.  Process-wide; on (non-zero) by
 * default; read when a launch is issued (a captured graph keeps the choice it was captured with).  The switch exists for
 * A/B timing and the parity tests. */
int pn2_set_sa_row_packing(int on);

/* pn2_linear(groups * 32, cin, cout, x, w, bias, relu = 1, pool = 32, y) on the LIVE rows only, for a pooled layer whose input
 * rows sit behind a ball query (the last layer of SA3: pointnet_util.py:150-170 on the un-pooled output of the fused chain):
 *   y[g] = relu( max_{j < 32} ( x[32 g + j] . w ) + bias )        x (groups * 32, cin)   idx (groups, 32)   y (groups, cout)
 * PRECONDITION, relied on for exactness: for every group g, the rows j >= live(g) of x equal row 0 of that group bit for bit,
 * live(g) = 1 + the last position of idx[g] that differs from position 0.  It holds for any x computed row by row by
 * deterministic kernels from rows gathered through idx (those rows gather the same source row).  The kernel classifies and
 * packs the groups as the row-packed set-abstraction kernels do and contracts each row in the k order of pn2_linear's LDS-tiled
 * kernel: y has the bits of pn2_linear(..., relu = 1, pool = 32) wherever that runs without a k split (from 4096 rows on for
 * cout = 256, from 8192 on for cout = 128).
 * Takes nsample = 32, relu = 1, a bias, cin % 4 == 0, cout % 128 == 0, x and w 16-byte aligned, and a 64-column slice of w
 * that fits the LDS (cin <= 576); with pn2_set_sa_row_packing(0), or anything else: PN2_EUNSUP, nothing launched (callers fall
 * back to pn2_linear). */
int pn2_linear_pool_packed(int groups, int nsample, int cin, int cout, const float *x, const int *idx, const float *w,
                           const float *bias, int relu, float *y, void *stream);

/* pn2_sa_mlp_max_fused / pn2_sa_mlp_rows_fused with the FEATURE part of the first layer hoisted by linearity:
 * [xyz - centre | features] @ W1 = (xyz - centre) @ W1[:3] + (features @ W1[3:])[idx], and zf = features @ W1[3:] has one
 * row per source point (b*n) instead of one per grouped neighbour (b*m*nsample).  zf (b*n, widths[0]) replaces `points`,
 * w[0] = the 3 xyz rows of the folded first-layer weight.  pool != 0: max over the neighbours -> (b, m, w_last); else the
 * un-pooled rows (b, m, nsample, w_last).  nsample = 32; widths multiples of 32, <= 128 ([64,64,128] pooled,
 * [128,128] un-pooled, [128,128,128] pooled); PN2_EUNSUP otherwise. */
int pn2_sa_mlp_fused_pre(int b, int n, int m, int nsample, const float *xyz, const float *new_xyz, const float *zf,
                         const int *idx, int nlayers, const int *widths, const float *const *w,
                         const float *const *bias, int pool, float *out, void *stream);

/* The wide-layer versions (pn2_fp_mlp_wide / pn2_sa_mlp_wide: widths 128 / 256 / 512, one launch per level) of the same
 * hoisting.  FP: z = points2 @ W0[:c2] (b*m, widths[0]); w[0] = the c1 skip-link rows of the folded first-layer weight
 * zero-padded to a multiple of 8 rows (c1 > 0, c1 % 4 == 0, n % 32 == 0).  SA: zf = points @ W0[feature rows]
 * (b*n, widths[0]); w[0] = the 3 xyz rows + 5 zero rows (8 x widths[0]); nsample = 32. */
int pn2_fp_mlp_wide_pre(int b, int n, int m, int c1, const float *dist, const int *idx, const float *points1,
                        const float *z, int nlayers, const int *widths, const float *const *w,
                        const float *const *bias, float *y, void *stream);
int pn2_sa_mlp_wide_pre(int b, int n, int m, int nsample, const float *xyz, const float *new_xyz, const float *zf,
                        const int *idx, int nlayers, const int *widths, const float *const *w,
                        const float *const *bias, int pool, float *y, void *stream);

/* query_ball_point with the binning hoisted out: pn2_ball_query_bin sorts every cloud of a batch into the uniform grid of
 * `radius` ONCE (one workgroup per cloud; workspace = b * pn2_ball_query_bin_bytes(n) bytes, 256-byte aligned, n <= 8192);
 * pn2_query_ball_point_binned then answers the queries from it -- its workgroups (16 per cloud at m = 1024) copy the
 * cell-sorted cloud instead of each re-binning it.  Same radius and xyz1 in both calls; results bit-identical to
 * pn2_query_ball_point (tf_grouping.cu:3-43).  PN2_EUNSUP for shapes outside the grid kernel (n > 8192, nsample > 64). */
size_t pn2_ball_query_bin_bytes(int n);
int pn2_ball_query_bin(int b, int n, float radius, const float *xyz1, void *workspace, size_t workspace_bytes, void *stream);
/* pn2_ball_query_bin with the cloud's rows ld1 floats apart (see pn2_fps_nested_ld): the bins of a dense copy, bit for bit.
 * pn2_query_ball_point_binned never reads xyz1 (the bins hold the cell-sorted cloud): it takes the strided pointer as it is. */
int pn2_ball_query_bin_ld(int b, int n, float radius, const float *xyz1, int ld1, void *workspace, size_t workspace_bytes,
                          void *stream);
int pn2_query_ball_point_binned(int b, int n, int m, float radius, int nsample, const float *xyz1, const float *xyz2,
                                const void *bins, int *idx, int *pts_cnt, int arith_mode, void *stream);

/* Pooling over the K neighbours of a group -- the `pooling=` variants of pointnet_sa_module, util/pointnet_util.py:165-191
 * (tf.reduce_max / reduce_mean / the exp(-5 |grouped_xyz|) weighted average / concat [avg, max]).  mode: 0 max, 1 avg,
 * 2 weighted_avg, 3 max_and_avg.  x (rows, k, c) float32, gxyz (rows, k, 3) (mode 2 only, else NULL) ->
 * out (rows, c), or (rows, 2c) = [avg | max] for mode 3.  The gradient is taken w.r.t. x only (grouped_xyz comes from
 * non-differentiable index ops); a maximum shared by several neighbours splits its gradient evenly (tf.reduce_max). */
int pn2_group_pool(long long rows, int k, int c, int mode, const float *x, const float *gxyz, float *out, void *stream);
int pn2_group_pool_grad(long long rows, int k, int c, int mode, const float *x, const float *gxyz, const float *dout,
                        float *dx, void *stream);

/* conv2d -> batch_norm -> relu -> conv2d of the training path (tf_util.py:186-204 twice) without writing the normalised
 * activation of the lower layer: pn2_bn_relu_forward_deferred turns the statistics of y (stats_done = 1: the
 * workspace is PN2_BN_WS_SUMMED; 0: PN2_BN_WS_ZEROED, the statistics are taken here) into save_mean / save_invstd, the moving
 * averages and per-channel (scale, shift) with z = relu?(fma(y, scale, shift)); pn2_linear_bn_stats_xf (the upper layer's
 * forward GEMM + statistics) and pn2_linear_wgrad_accumulate_xf (its weight gradient) apply them to y while loading it.
 * Only valid when the lower activation has no other consumer.  _xf: cin % 4 == 0, rows > 2048, 16-byte aligned operands,
 * else PN2_EUNSUP. */
int pn2_bn_relu_forward_deferred(long long rows, int c, const float *y, const float *gamma, const float *beta,
                                 const float *bias, float eps, float decay, int stats_done, float *running_mean,
                                 float *running_var, void *workspace, size_t workspace_bytes, float *save_mean,
                                 float *save_invstd, float *scale, float *shift, void *stream);
int pn2_linear_bn_stats_xf(int rows, int cin, int cout, const float *x_raw, const float *w, float *y, void *bn_workspace,
                           size_t workspace_bytes, const float *a_scale, const float *a_shift, int a_relu, void *stream);
int pn2_linear_wgrad_accumulate_xf(int rows, int cin, int cout, const float *x_raw, const float *dy, float *dw,
                                   const float *a_scale, const float *a_shift, int a_relu, void *stream);

/* y (rows, cout) = x (rows, cin) . w (cin, cout) + bias (NULL: none), no activation, for 1 <= cout <= 16: the class head
 * (model.py:145-146: conv1d(num_class), activation_fn=None) as one streaming launch instead of a zero-padded MFMA layer.
 * cin % 4 == 0, cin * cout * 4 <= 48 KB, x 16-byte aligned, else PN2_EUNSUP. */
int pn2_linear_narrow(int rows, int cin, int cout, const float *x, const float *w, const float *bias, float *y, void *stream);

/* The batch-norm gradient of the training path (tf_util.py:555-581 through tf.gradients) applied ON LOAD by the two gradient
 * GEMMs of the layer, so that dy = the gradient leaving the batch norm (+ReLU [+ max over groups of 32 rows]) is never written
 * or re-read.  pn2_bn_grad_constants turns the two per-channel sums (stats_done = 1: the workspace is
 * PN2_BN_WS_SUMMED by the data gradient of the layer above; 0: PN2_BN_WS_ZEROED, the sums are taken here with one pass over
 * (dz, y)) into dgamma, dbeta and coef (6, c) = sc, sh, mean, invstd, k1, k2 with
 * dy = sc * fma(-(y - mean) * invstd, k2, g - k1), g = dz * [relu mask] -- pn2_bn_relu_backward's expressions, so both forms
 * hand the GEMMs the same bits.  pn2_linear_dgrad_gx: dx (rows, cin) = dy (rows, cout) . W^T (pn2_linear_dgrad) with dy formed
 * from y (rows, cout), dz ((rows, cout); pool = 32: the (rows / 32, cout) gradient of the pooled maxima beside zmax / ties of
 * pn2_bn_relu_forward) and coef; y_below != NULL adds pn2_linear_dgrad_bn_grad_stats' epilogue for the layer below.
 * pn2_linear_wgrad_gx: dw (cin, cout) += x^T . dy likewise; a_scale != NULL: x is the pre-normalisation output of the layer
 * below (pn2_linear_wgrad_accumulate_xf).  pool in {0, 32}; cout % 4 == 0, 16 < cout <= 512 and 16-byte aligned y / dz / coef for
 * the data gradient, else PN2_EUNSUP. */
int pn2_bn_grad_constants(long long rows, int c, const float *dz, const float *y, const float *gamma, const float *beta,
                          const float *save_mean, const float *save_invstd, int relu, int pool, const float *zmax,
                          const float *ties, const float *ysel, int stats_done, void *workspace, size_t workspace_bytes,
                          float *coef, float *dgamma, float *dbeta, void *stream);
/* pn2_bn_relu_forward with pool > 1 that also keeps ysel (rows / pool, c) = the pre-normalisation value of the first row that
 * attains each pooled maximum.  With it (pn2_bn_grad_constants(..., ysel != NULL, stats_done = 0)) the backward reduction behind
 * the max pool reads the pooled tensors only -- the gradient is non-zero on the rows attaining the maximum, all of which carry
 * zmax -- instead of making a pass over y (rows, c).  pool > 1 and ysel are required; stats_mode: a PN2_BN_WS_* state. */
int pn2_bn_relu_forward_pool(long long rows, int c, const float *y, const float *gamma, const float *beta, const float *bias,
                             float eps, float decay, int relu, int pool, float *running_mean, float *running_var,
                             void *workspace, size_t workspace_bytes, int stats_mode, float *save_mean, float *save_invstd,
                             float *zmax, float *ties, float *ysel, void *stream);
int pn2_linear_dgrad_gx(int rows, int cin, int cout, const float *y, const float *dz, const float *coef, int relu, int pool,
                        const float *zmax, const float *ties, const float *w, float *dx, const float *y_below,
                        const float *gamma_below, const float *beta_below, const float *mean_below, const float *invstd_below,
                        int relu_below, void *ws_below, size_t ws_below_bytes, void *stream);
int pn2_linear_wgrad_gx(int rows, int cin, int cout, const float *x, const float *a_scale, const float *a_shift, int a_relu,
                        const float *y, const float *dz, const float *coef, int relu, int pool, const float *zmax,
                        const float *ties, float *dw, void *stream);

/* "The last workgroup finishes" (round 6): every producer of batch-norm sums used to be followed by a one-block launch that folds
 * the slot copies of the sums and derives per-channel constants (45 launches of ~5 us per training step, all on the critical
 * path).  The producers below take a two-level ticket per workgroup instead, and the workgroup that draws the last one does that
 * work inside the producing launch.
 *   pn2_linear_bn_stats_fin: pn2_linear_bn_stats (a_scale == NULL) / pn2_linear_bn_stats_xf + finish 1: fold (the
 *     workspace is then PN2_BN_WS_FOLDED for pn2_bn_relu_forward_mode / pn2_bn_relu_forward_pool), or 2: fold + what
 *     pn2_bn_relu_forward_deferred publishes (save_mean, save_invstd, moving averages, scale / shift; both NULL: not wanted).
 *   pn2_linear_dgrad_fin: pn2_linear_dgrad (dy given, y == NULL) / pn2_linear_dgrad_gx (dy == NULL) + the epilogue of
 *     pn2_linear_dgrad_bn_grad_stats for the layer below (y_below != NULL) + finish_below 0: none, 1: fold (the
 *     workspace is then PN2_BN_WS_FOLDED for pn2_bn_relu_backward_mode), 3: fold + what pn2_bn_grad_constants publishes there.
 *   pn2_bn_relu_forward_mode / pn2_bn_relu_backward_mode: pn2_bn_relu_forward (pool = 0) / pn2_bn_relu_backward with the state
 *     of the workspace given as stats_mode (a PN2_BN_WS_* state; SUMMED and FOLDED need pool <= 1 in the backward).
 * (pn2_bn_relu_forward_deferred and pn2_bn_grad_constants with stats_done = 0 and the UNCLEARED / ZEROED batch-norm calls
 * finish inside their own reduction kernel; no signature changes.)  Reference: tf_util.py:186-204,555-581. */
int pn2_linear_bn_stats_fin(int rows, int cin, int cout, const float *x, const float *w, float *y, void *bn_workspace,
                            size_t workspace_bytes, const float *a_scale, const float *a_shift, int a_relu, int finish,
                            const float *gamma, const float *beta, const float *bias, float eps, float decay,
                            float *running_mean, float *running_var, float *save_mean, float *save_invstd, float *scale,
                            float *shift, void *stream);
int pn2_linear_dgrad_fin(int rows, int cin, int cout, const float *dy, const float *y, const float *dz, const float *coef,
                         int relu, int pool, const float *zmax, const float *ties, const float *w, float *dx,
                         const float *y_below, const float *gamma_below, const float *beta_below, const float *mean_below,
                         const float *invstd_below, int relu_below, void *ws_below, size_t ws_below_bytes, int finish_below,
                         float *coef_below, float *dgamma_below, float *dbeta_below, void *stream);
int pn2_bn_relu_forward_mode(long long rows, int c, const float *y, const float *gamma, const float *beta, const float *bias,
                             float eps, float decay, int relu, float *running_mean, float *running_var, void *workspace,
                             size_t workspace_bytes, int stats_mode, float *save_mean, float *save_invstd, float *z,
                             void *stream);
int pn2_bn_relu_backward_mode(long long rows, int c, const float *dz, const float *y, const float *gamma, const float *beta,
                              const float *save_mean, const float *save_invstd, int relu, int pool, const float *zmax,
                              const float *ties, void *workspace, size_t workspace_bytes, int stats_mode, float *dy,
                              float *dgamma, float *dbeta, void *stream);

/* Data gradient AND weight gradient of a narrow dense + batch-norm layer in ONE launch (csrc/pn2_bwd_fused.hip): what
 * pn2_linear_dgrad_fin and pn2_linear_wgrad_gx compute for the same arguments -- dx (rows, cin) = dy . W^T, dw (cin, cout) +=
 * x^T . dy with dy = the gradient leaving the layer's batch norm formed on load from (y, dz, coef), the epilogue and finish for
 * the layer below -- reading (y, dz) ONCE: for 32 / 64-channel layers over 10^5 .. 10^6 rows both GEMMs are HBM streams and the
 * second read is a third of the traffic.  cin, cout in {32, 64}, rows % 32 == 0, 16-byte aligned operands, else PN2_EUNSUP.
 * dw is added to.  tf_util.py:181-204,555-581 through tf.gradients. */
int pn2_linear_bwd_fused(int rows, int cin, int cout, const float *x, const float *a_scale, const float *a_shift, int a_relu,
                         const float *y, const float *dz, const float *coef, int relu, int pool, const float *zmax,
                         const float *ties, const float *w, float *dx, float *dw, const float *y_below,
                         const float *gamma_below, const float *beta_below, const float *mean_below, const float *invstd_below,
                         int relu_below, void *ws_below, size_t ws_below_bytes, int finish_below, float *coef_below,
                         float *dgamma_below, float *dbeta_below, void *stream);

/* First layer of an SA module whose points carry few channels (c <= 5: xyz + rgb of the level-0 module), training path, in ONE
 * launch: y (b,m,nsample,cout) = [group_point(xyz, idx) - new_xyz | group_point(points, idx)] . w (3 + c, cout)
 * (pointnet_util.py:39-54 + tf_util.py:181-186) written once, its batch statistics taken on the way out into the ZEROED
 * workspace and folded by the launch's last workgroup (finish 1) or folded and turned into the deferred batch norm's constants
 * (finish 2, see pn2_linear_bn_stats_fin).  xg (b,m,nsample,3+c), optional: the grouped input for the weight gradient. */
int pn2_sa_first_layer_bn(int b, int n, int m, int nsample, int c, int cout, const float *xyz, const float *new_xyz,
                          const float *points, const int *idx, const float *w, float *y, float *xg, void *workspace,
                          size_t workspace_bytes, int finish, const float *gamma, const float *beta, const float *bias, float eps,
                          float decay, float *running_mean, float *running_var, float *save_mean, float *save_invstd,
                          float *scale, float *shift, void *stream);

/* First layer of an SA / FP module of the TRAINING path with its feature half applied to the source rows (gather and
 * interpolation are linear and commute with a 1x1 conv):
 *   SA (pointnet_util.py:39-54,150-156):  y (b,m,nsample,cout) = (group_point(xyz, idx) - new_xyz) . w_xyz (3,cout) + z[b, idx]
 *      with z (b,n,cout) = points . W[3:] from pn2_linear; gxyz (b,m,nsample,3), optional: the centred coordinates.
 *   FP (pointnet_util.py:300-312):        y (b,n,cout) = three_interpolate(z, idx, w(dist)) + points1 (b,n,c1) . w1 (c1,cout)
 *      with z (b,m,cout) = points2 . W[:c2]; weights from three_nn's squared distances as in pn2_fp_interp_concat; 1 <= c1 <= 8.
 * cout % 4 == 0, <= 1024; z, y, w 16-byte aligned.  The data and weight gradients of the feature half are then GEMMs over
 * the source rows (pn2_scatter_plan_apply of dy -> dz, pn2_linear_dgrad / pn2_linear_wgrad on n resp. m rows). */
int pn2_sa_hoist_rows(int b, int n, int m, int nsample, int cout, const float *xyz, const float *new_xyz, const int *idx,
                      const float *z, const float *w_xyz, float *y, float *gxyz, void *stream);
int pn2_fp_hoist_rows(int b, int n, int m, int c1, int cout, const float *dist, const int *idx, const float *points1,
                      const float *z, const float *w1, float *y, void *stream);
/* The same two with the batch statistics of y (tf_util.py:186-204: conv2d -> batch_norm_template) taken on the way out: every
 * workgroup adds its column sums of y and y^2 (fp64) to one of the slot copies of the ZEROED batch-norm workspace
 * (pn2_bn_workspace_bytes(cout)), so no statistics pass reads y again; finish = 0: the copies are left there
 * (PN2_BN_WS_SUMMED), 1: the last workgroup folds them (PN2_BN_WS_FOLDED), 2: it also publishes what
 * pn2_bn_relu_forward_deferred publishes (save_mean / save_invstd, the moving averages, scale / shift) -- the arguments of
 * pn2_linear_bn_stats_fin.  r06: the hoisted first layers of SA2-SA4 / FP4 in training are one launch less each. */
int pn2_sa_hoist_rows_bn(int b, int n, int m, int nsample, int cout, const float *xyz, const float *new_xyz, const int *idx,
                         const float *z, const float *w_xyz, float *y, float *gxyz, void *bn_workspace, size_t workspace_bytes,
                         int finish, const float *gamma, const float *beta, const float *bias, float eps, float decay,
                         float *running_mean, float *running_var, float *save_mean, float *save_invstd, float *scale,
                         float *shift, void *stream);
int pn2_fp_hoist_rows_bn(int b, int n, int m, int c1, int cout, const float *dist, const int *idx, const float *points1,
                         const float *z, const float *w1, float *y, void *bn_workspace, size_t workspace_bytes, int finish,
                         const float *gamma, const float *beta, const float *bias, float eps, float decay, float *running_mean,
                         float *running_var, float *save_mean, float *save_invstd, float *scale, float *shift, void *stream);
/* pn2_sa_hoist_rows_bn for nscales (<= 4) scales of one batch in ONE launch -- the first layers of pointnet_sa_module_msg
 * (pointnet_util.py:219-282) in training, whose scales all gather from the same cloud:
 *   y[s] (b,m,nsample[s],cout[s]) = z[b, idx[s], zcol[s] : zcol[s] + cout[s]] + (group_point(xyz, idx[s]) - new_xyz) . w_xyz[s]
 * z (b,n,z_stride) = points . [Wf_0 | Wf_1 | ...] is ONE product of the caller (pn2_linear), read in place by column block;
 * gxyz[s] (b,m,nsample[s],3), optional (null table or null entry): the centred coordinates.  The batch statistics of y[s] go to
 * bn_workspace[s] (ZEROED, workspace_bytes[s] >= pn2_bn_workspace_bytes(cout[s])); finish[s] = 0 / 1 / 2 and the tables gamma ..
 * shift as the arguments of pn2_sa_hoist_rows_bn (a null table = a table of nulls), eps / decay shared.  Every per-scale argument
 * is a host array read at call time (as pn2_multi_copy's), so the call may be captured.  y[s] and gxyz[s] are the bits of
 * pn2_sa_hoist_rows on a dense copy of the scale's columns.  cout[s] % 4 == 0, <= 1024 (PN2_EUNSUP); zcol[s] % 4 == 0,
 * z_stride % 4 == 0, z / y[s] / w_xyz[s] 16-byte aligned (PN2_EINVAL). */
int pn2_sa_hoist_rows_multi_bn(int nscales, int b, int n, int m, int z_stride, const float *xyz, const float *new_xyz, const float *z,
                               const int *nsample, const int *cout, const int *zcol, const int *const *idx,
                               const float *const *w_xyz, float *const *y, float *const *gxyz, void *const *bn_workspace,
                               const size_t *workspace_bytes, const int *finish, const float *const *gamma,
                               const float *const *beta, const float *const *bias, float eps, float decay,
                               float *const *running_mean, float *const *running_var, float *const *save_mean,
                               float *const *save_invstd, float *const *scale, float *const *shift, void *stream);

/* ---- raw ASCII scans: the step in front of the down-sampling (reference preprocess.py:23-55, util/point_cloud_util.py:53-57) ----
 * Semantic3D ships <scene>.txt (`x y z intensity r g b` per line) and <scene>.labels (one integer per line).  Both are parsed
 * from a device buffer of text in two stages: a line index, then one line per lane.  One call takes one chunk of at most
 * PN2_TEXT_MAX_BYTES bytes (int offsets), 16-byte aligned, holding whole lines; lines end in '\n', a last line without one
 * is a line, nothing follows a final '\n'.  Tokens are separated by runs of space, tab and '\r'.
 *
 * Number rule (the oracle is Python's float(token) / int(token) on the grammar below):
 *   float token  [+-]? digits* ('.' digits*)? ([eE][+-]?digits+)?  with at least one mantissa digit.  With leading zeros
 *                stripped, w = the integer of ALL mantissa digits and e10 = exponent - number of fraction digits:
 *                w <= 2^53 and |e10| <= 22 is FAST: the value is (double)w * 10^e10 or (double)w / 10^-e10 -- one correctly
 *                rounded IEEE operation on two exact operands (Clinger's fast path), equal to float(token); -0.0 keeps its
 *                sign.  Every other valid token, and nan / inf / infinity in any case with an optional sign, is SLOW: the
 *                column's bit (1 << column) is set in the line's flags and nothing is written for it (the caller parses it).
 *   int token    [+-]?digits+ with the value in int32; anything else makes the line malformed.
 * Column kinds: PN2_TEXT_F64 -> the next column of out_f64 (nlines, nF); PN2_TEXT_I32 (int token) and PN2_TEXT_TRUNC_I32
 * (float token truncated toward zero, the reference's int(float(tok)); |v| >= 2^31 makes the line malformed) -> the next
 * column of out_i32 (nlines, nI); PN2_TEXT_SKIP: any token, not read.  A line with another number of tokens than ncols, a
 * bad token or nothing but whitespace is malformed: PN2_TEXT_MALFORMED in its flags, its outputs unspecified. */
#define PN2_TEXT_TILE_BYTES 4096     /* bytes of text per workgroup of the line index: 256 lanes x one 16-byte load */
#define PN2_TEXT_MAX_BYTES 1073741824
#define PN2_TEXT_MAX_COLS 8
#define PN2_TEXT_F64 0
#define PN2_TEXT_I32 1
#define PN2_TEXT_TRUNC_I32 2
#define PN2_TEXT_SKIP 3
#define PN2_TEXT_MALFORMED 128       /* the flags' top bit; column 7, where there is one, is therefore I32 or SKIP (PN2_EUNSUP) */

/* Line index.  line_start (line_cap) int32: entry i = offset of the first byte of line i, entry nlines = one past the '\n'
 * that ends the last line (nbytes + 1 when it has none), so line i is [line_start[i], line_start[i + 1] - 1).  *out_count
 * (device int) = nlines, whatever line_cap is; entries at or past line_cap are not written, so a caller that finds
 * *out_count + 1 > line_cap calls again with more room.  workspace: 256-byte aligned, *bytes of
 * pn2_text_index_workspace_bytes(nbytes) -- per tile of PN2_TEXT_TILE_BYTES a count and its exclusive scan. */
int pn2_text_index_workspace_bytes(int nbytes, unsigned long long *bytes);
int pn2_text_index_lines(const unsigned char *text, int nbytes, int *line_start, int line_cap, int *out_count,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Field parse of lines [0, nlines) of the index above.  kinds (ncols) is a HOST array of PN2_TEXT_* read at call time.
 * out_f64 / out_i32 may be NULL when no column writes there.  flags (nlines) bytes.  status (3) device ints, set by the
 * call: the smallest malformed line index (0x7fffffff: none), the number of malformed lines, the number of slow tokens
 * in well-formed lines.  Needs no workspace. */
int pn2_text_parse(const unsigned char *text, int nbytes, const int *line_start, int nlines, const int *kinds, int ncols,
                   double *out_f64, int *out_i32, unsigned char *flags, int *status, void *stream);

/* ---- scene files: what the predict flow writes and reads back (reference util/point_cloud_util.py:60-63, Open3D's .pcd) ----
 * Integer text, the inverse of pn2_text_parse with PN2_TEXT_I32 columns.  values (nrows, ncols) int32, row-major,
 * 1 <= ncols <= PN2_TEXT_MAX_COLS.  A row becomes its tokens as Python's "%d" prints them (a '-' for negatives, no '+', no
 * leading zeros; INT32_MIN included), separated by one space, ended by '\n'.  *out_bytes (device u64) = the bytes all rows
 * need, whatever text_cap is; text[0 : min(need, text_cap)) is exactly that prefix of the full text; no byte at or past
 * text_cap and no byte past need is written, so a caller whose buffer holds nrows * ncols * PN2_TEXT_I32_CHARS bytes never
 * calls twice.  text: 16-byte aligned; nrows * ncols * PN2_TEXT_I32_CHARS <= PN2_TEXT_MAX_BYTES (int offsets, PN2_ERANGE).
 * One row per lane, PN2_TEXT_FORMAT_ROWS rows per workgroup: row lengths and a total per workgroup, an exclusive scan of the
 * totals, then every workgroup stages its contiguous span in LDS and stores it 16 bytes at a time.  workspace: 256-byte
 * aligned, *bytes of pn2_text_format_workspace_bytes(nrows) -- per workgroup a total and its scan. */
#define PN2_TEXT_I32_CHARS 12        /* most bytes of one token with its separator: "-2147483648" and a ' ' or '\n' */
#define PN2_TEXT_FORMAT_ROWS 256
int pn2_text_format_workspace_bytes(int nrows, unsigned long long *bytes);
int pn2_text_format_i32(const int *values, int nrows, int ncols, unsigned char *text, size_t text_cap,
                        unsigned long long *out_bytes, void *workspace, size_t workspace_bytes, void *stream);

/* The payload of a binary .pcd with 4-byte fields, one row per lane.  n <= PN2_PCD_MAX_ROWS (PN2_ERANGE); rows 16-byte aligned.
 * pn2_pcd_pack: points (n,3) float32 (PN2_PCD_F32) or float64 (PN2_PCD_F64) -> rows of `x y z` (12 bytes, PN2_PCD_COLOR_NONE)
 * or `x y z rgb` (16 bytes), what util.point_cloud_util.write_point_cloud_pcd writes: coordinates (float)p, the colour word
 * (r << 16) | (g << 8) | b with r = clip(floor(c * 255.0), 0, 255) of a float64 colour in [0, 1] (PN2_PCD_COLOR_F64, (n,3)) or
 * the byte itself (PN2_PCD_COLOR_U8, (n,3)).
 * pn2_pcd_unpack: rows of nfields (3 .. PN2_PCD_MAX_FIELDS) words, ix / iy / iz / irgb the word index of each field
 * (irgb = -1: none) -> points (n,3) float64 = the words read as float32, colors (n,3) float64 = byte / 255.0 correctly rounded
 * (zeros without an rgb field; colors = NULL: not written) -- util.point_cloud_util.read_point_cloud_pcd's arrays. */
#define PN2_PCD_F32 0
#define PN2_PCD_F64 1
#define PN2_PCD_COLOR_NONE 0
#define PN2_PCD_COLOR_F64 1
#define PN2_PCD_COLOR_U8 2
#define PN2_PCD_MAX_ROWS 134217728
#define PN2_PCD_MAX_FIELDS 64
int pn2_pcd_pack(const void *points, int point_kind, const void *colors, int color_kind, int n, unsigned int *rows,
                 void *stream);
int pn2_pcd_unpack(const unsigned int *rows, int n, int nfields, int ix, int iy, int iz, int irgb, double *points,
                   double *colors, void *stream);

/* ---- records: rows of any byte stride with typed fields at any byte offset (csrc/pn2_records.hip) -- the payload of a binary
 * .ply, and of a .pcd whose fields have any SIZE / TYPE / COUNT.  A record is `stride` bytes, 1 <= stride <=
 * PN2_REC_MAX_STRIDE (PN2_EUNSUP above), n * stride <= PN2_REC_MAX_BYTES (int offsets, PN2_ERANGE).  Seven slots describe the
 * fields: x y z c0 c1 c2 label, each with a byte offset (-1: absent) and a type code PN2_REC_*; offsets and types are HOST
 * int[PN2_REC_SLOTS] arrays read at call time.  flags: PN2_REC_BIG_ENDIAN (the fields are big-endian), PN2_REC_FORM_PLAIN (run
 * the row-per-lane form even where the staged one applies: same bytes, for tests and measurements).
 * pn2_record_unpack -> points (n,3) float64: the value of x y z, exact (every type is a subset of float64).
 *   colors (n,3) float64, NULL: not written.  PN2_REC_COLOUR_NONE: zeros.  PN2_REC_COLOUR_THREE: channels c0 c1 c2.
 *   PN2_REC_COLOUR_PACKED: one 4-byte word in c0 holding 0x00RRGGBB (PCD's rgb / rgba), each byte / 255.0.  The channel rules
 *   are THIS PROJECT'S OWN DEFINITION, not a standard's: a U8 channel is byte / 255.0 correctly rounded (pn2_pcd_unpack's rule),
 *   a U16 channel v / 65535.0, an F32 / F64 channel the value itself; other integer types PN2_EUNSUP.
 *   labels (n) int32, NULL: not written.  An integer field converted to int32 (U32 reinterpreted).  A float field must be finite,
 *   integral and inside int32; otherwise the label is 0 and *invalid (device int64, ADDED to; required for a float label) goes
 *   up by one.
 *   A slot is read only where its output is asked for: x y z always, the colour slots with colors, the label with labels.
 * pn2_record_pack: the inverse for the layouts the writers need -- x y z as coord_type PN2_REC_F32 ((float)p) or PN2_REC_F64
 *   from points (n,3) PN2_PCD_F32 / PN2_PCD_F64; then, with color_kind PN2_PCD_COLOR_U8 / _F64, three U8 channels (the byte
 *   itself / clip(floor(c * 255.0), 0, 255), a NaN 0: pn2_pcd_pack's rule); then, with labels != NULL, an I32.  Tightly packed
 *   in that order, little-endian: stride 12 / 24 + 3 + 4.
 * Checks in this order: n, stride, kinds and flags PN2_EINVAL; stride above the limit PN2_EUNSUP; NULL pointers PN2_ENULL;
 * PN2_ERANGE; then PN2_EINVAL for an unknown type code, a wanted field that is absent or reaches past stride, two wanted fields
 * that overlap, rows not 16-byte aligned, an output not naturally aligned.
 * Memory: global memory is touched with naturally aligned accesses only; unpack reads no byte at or past n * stride rounded up
 * to 16, pack writes no byte at or past n * stride.  Strides up to PN2_REC_STAGE_BYTES / 64 go through LDS in 16-byte pieces. */
#define PN2_REC_U8 0
#define PN2_REC_I8 1
#define PN2_REC_U16 2
#define PN2_REC_I16 3
#define PN2_REC_U32 4
#define PN2_REC_I32 5
#define PN2_REC_F32 6
#define PN2_REC_F64 7
#define PN2_REC_BIG_ENDIAN 1
#define PN2_REC_FORM_PLAIN 2
#define PN2_REC_COLOUR_NONE 0
#define PN2_REC_COLOUR_THREE 1
#define PN2_REC_COLOUR_PACKED 2
#define PN2_REC_SLOTS 7
#define PN2_REC_MAX_STRIDE 1024
#define PN2_REC_MAX_BYTES 2147483632 /* 2^31 - 16 */
#define PN2_REC_STAGE_BYTES 32768
int pn2_record_unpack(const void *rows, int n, int stride, const int *offsets, const int *types, int colour_kind, int flags,
                      double *points, double *colors, int *labels, long long *invalid, void *stream);
int pn2_record_pack(const void *points, int point_kind, const void *colors, int color_kind, const int *labels, int n,
                    int coord_type, int flags, void *rows, void *stream);

/* ---- point-cloud augmentation: util/provider.py of the reference as one pipeline (csrc/pn2_augment.hip) ------------------
 * in (b,n,c) float32 -> out (b,n,c) float32, c >= 3, xyz in channels 0:3; in_labels (b,n) int32 -> out_labels and in_weights
 * (b,n) float32 -> out_weights are optional companions (both of a pair or neither) that are only ever permuted.  Stages run
 * in this fixed order; `flags` turns each on by its bit:
 *   0 PN2_AUG_SHUFFLE   shuffle_points: out row j is in row perm[j], ONE permutation (n) for the whole batch; labels and
 *                       weights follow.  Every later stage, and every per-point draw, is indexed by the row after the shuffle.
 *   1 PN2_AUG_ROTATE | PN2_AUG_PERTURB   p @ R for a (3,3) matrix R per cloud (rotate_point_cloud, rotate_feature_point_cloud,
 *                       rotate_point_cloud_with_normal, rotate_point_cloud_by_angle*, rotate_perturbation_point_cloud*); with
 *                       PN2_AUG_ROTATE_NORMALS (needs c >= 6) channels 3:6 are rotated by the same R.
 *   2 PN2_AUG_SCALE     random_scale_point_cloud: xyz * s, one s per cloud.
 *   3 PN2_AUG_SHIFT     shift_point_cloud: xyz + t, one t (3) per cloud.
 *   4 PN2_AUG_JITTER    jitter_point_cloud: x + clip(jitter_sigma * z, -jitter_clip, jitter_clip), one standard normal z per
 *                       value: xyz only (cj = 3) -- with PN2_AUG_JITTER_ALL all c channels (cj = c), as the reference does to
 *                       the (B,N,3) arrays it is given.
 *   5 PN2_AUG_DROPOUT   random_point_dropout: row j of a cloud with u[j] <= ratio becomes row 0 of that cloud as it leaves
 *                       stage 4 (all c channels).  A dropped row reads nobody's output: it redoes stages 1-4 on the INPUT of row
 *                       0 with row 0's own jitter draws; row 0, dropped or not, keeps its own value.  Labels and weights are
 *                       not touched (the reference does not touch them).
 * Arithmetic rule.  An enabled stage takes float64 and does the reference's one operation in float64: rotation
 * (x*R[0][j] + y*R[1][j]) + z*R[2][j] in that order (the library is built with -ffp-contract=off), scale x*s, shift x + t,
 * jitter x + clip(sigma*z).  The float32 input is widened once, values stay float64 between enabled stages and are rounded to
 * float32 once, at the store.  With ONE stage enabled this is what the numpy function does to a float32 batch (numpy computes
 * `f32 op= f64` and np.dot of a float32 array with a float64 matrix in float64 and rounds once).  Scale and shift act on xyz,
 * rotation on xyz (and 3:6 with PN2_AUG_ROTATE_NORMALS); a channel no enabled stage touches is copied unchanged.
 *
 * Draws, replay mode (flags & PN2_AUG_REPLAY): the device forms none; per enabled stage its input is required (PN2_ENULL):
 * draw_perm (n) int32 (an entry outside [0,n) reads row j itself), draw_matrix (b,3,3) float64, draw_scale (b), draw_shift
 * (b,3), draw_noise (b,n,cj) float64 standard normals (before sigma and the clip), draw_ratio (b) and draw_u (b,n) float64.
 * counter is not read.
 * Draws, device mode: counter-based hashes of csrc/pn2_rng.h.  h(s) = sample_stream(seed, *counter, s) for cloud s, draw i of
 * it U(i) = unit53(draw64(h(s), i)) in [0,1), and
 *   uniform(lo, hi) = lo + (hi - lo) * U;  angle = (U * 2.0) * pi;
 *   normal(i) = sqrt(-2.0 * log(1.0 - U(i))) * cos((U(i + 1) * 2.0) * pi)   (Box-Muller, float64)
 * with these indices (T = 2^41):
 *   T + 0          rotation angle about rotate_axis (0 x, 1 y, 2 z: the reference's three matrices)      [PN2_AUG_ROTATE]
 *   T + 2 + 2k     k = 0,1,2: normal -> angle_k = clip(perturb_sigma * normal, -perturb_clip, perturb_clip); R_perturb =
 *                  Rz . (Ry . Rx) as the reference builds it; with both bits R = R_axis . R_perturb; every 3x3 product in
 *                  the plain order (a0*b0 + a1*b1) + a2*b2                                               [PN2_AUG_PERTURB]
 *   T + 8          scale = uniform(scale_lo, scale_hi)
 *   T + 9 + a      shift[a] = uniform(-shift_range, shift_range), a = 0,1,2
 *   T + 12         ratio = U * dropout_max
 *   2T + 2*(j*cj + a)   normal of the jitter of row j, channel a
 *   4T + j         u[j] of the dropout of row j
 *   and for the permutation the stream of cloud index -1: key[i] = draw64(h(-1), 8T + i); perm = the indices sorted by
 *   (key, index), i.e. perm[rank of i] = i.
 * *counter (device int64) is read once and advanced by one per call, by a one-workgroup prologue launch that snapshots it
 * into the workspace and forms the per-cloud parameters; the other launches read the snapshot.  No host synchronisation; a
 * captured call replays into fresh draws.  Launches: prologue, permutation (rank count over LDS tiles of keys, only with
 * PN2_AUG_SHUFFLE), rows (256 lanes, grid (row tiles, b), one row per lane).
 * Outputs: out_params (b,PN2_AUG_PARAMS) float64 = R (9, row-major), scale, shift (3), ratio, 0, 0 of this call (identity /
 * 1 / 0 / 0 for a stage that is off), or NULL; out_perm (n) int32, required with PN2_AUG_SHUFFLE.
 * in == out is allowed without PN2_AUG_SHUFFLE (PN2_EINVAL with it; PN2_EUNSUP with PN2_AUG_DROPOUT and c >
 * PN2_AUG_INPLACE_MAX_C: row 0 of every cloud is then kept in the workspace).  Labels / weights may alias their outputs likewise.
 * PN2_EINVAL: b, n <= 0, c < 3, b > 65535, unknown flag bits or axis, PN2_AUG_ROTATE_NORMALS with c < 6, a stage's parameters
 * out of order (sigma < 0, clip <= 0, lo > hi, range < 0, dropout_max outside [0,1]), workspace too small or not 256-byte
 * aligned; PN2_ENULL: in, out, workspace, counter (device mode), a replay input of an enabled stage, out_perm with shuffle. */
#define PN2_AUG_SHUFFLE 1
#define PN2_AUG_ROTATE 2
#define PN2_AUG_PERTURB 4
#define PN2_AUG_SCALE 8
#define PN2_AUG_SHIFT 16
#define PN2_AUG_JITTER 32
#define PN2_AUG_DROPOUT 64
#define PN2_AUG_ROTATE_NORMALS 128
#define PN2_AUG_JITTER_ALL 256
#define PN2_AUG_REPLAY 512
#define PN2_AUG_PARAMS 16
#define PN2_AUG_INPLACE_MAX_C 64
int pn2_augment_workspace_bytes(int b, unsigned long long *bytes);
int pn2_augment(int b, int n, int c, int flags, int rotate_axis, double perturb_sigma, double perturb_clip, double scale_lo,
                double scale_hi, double shift_range, double jitter_sigma, double jitter_clip, double dropout_max,
                unsigned long long seed, long long *counter, const int *draw_perm, const double *draw_matrix,
                const double *draw_scale, const double *draw_shift, const double *draw_noise, const double *draw_ratio,
                const double *draw_u, const float *in, const int *in_labels, const float *in_weights, void *workspace,
                size_t workspace_bytes, double *out_params, int *out_perm, float *out, int *out_labels, float *out_weights,
                void *stream);

/* The per-frame front end of the KITTI flow (csrc/pn2_frame.hip): dataset/kitti_dataset.py:15-26 and :40-54 of the reference.
 * Between the two calls the cropped frame is x-sorted by pn2_scene_ingest (stable, with out_perm).
 *
 * pn2_frame_crop: frame = n rows of float32, row stride row_floats >= 3 floats, x y z first (a KITTI .bin row is x y z intensity:
 * row_floats = 4).  A row is kept iff lo <= p <= hi on all three axes, compared in float64, INCLUSIVE on both sides (the project's
 * definition of Open3D's crop_point_cloud); a NaN or +-inf coordinate drops its row by the comparison.  Kept rows
 * stay in frame order: out_points (n,3) float64 = the float32 values widened exactly, out_src (n) int32 = the frame row of each,
 * *out_count (device int32) = how many; rows [count, n) of both outputs are not written.  Two launches, no host
 * synchronisation.  workspace: 256-byte aligned, pn2_frame_crop_workspace_size(n) bytes (one sized for n serves any smaller n),
 * nothing kept between calls.  n <= PN2_FRAME_MAX_ROWS, else PN2_ERANGE.
 *
 * pn2_frame_sample: points (cnt,3) float64, the cropped frame sorted by x; one sample of npts points of the whole frame.
 *   cnt <= npts          out_sel[j] = j mod cnt (the reference's doubling loop; cnt == npts takes this branch, unshuffled).
 *   cnt > npts, mask     replay: mask = cnt bytes, the reference's shuffled boolean mask; out_sel = its set positions, ascending.
 *                        A mask that does not select exactly npts: status PN2_FRAME_ST_MASK.
 *   cnt > npts, no mask  the npts smallest of the keys draw64(sample_stream(seed, *counter, 0), i), i in [0, cnt), ties broken
 *                        by index, emitted in ascending index order (csrc/pn2_rng.h; the subset-key index space of
 *                        pn2_dataset_sample).  PN2_FRAME_ST_CAND: more than 4096 keys share the deciding 12-bit bin (about
 *                        cnt / 4096 are expected).
 *   mask == NULL (either count): the last launch advances *counter (device int64) by one, so a captured call replays into fresh
 *   subsets.  With a mask, counter is not touched and may be NULL.
 * box_min = the float64 minimum over the SAMPLED points; shift = (min_x + box_size_x / 2, min_y + box_size_y / 2, min_z);
 * out_centered (npts,3) float32 = float32(p - shift), the subtraction in float64; out_raw (npts,3) float64 = the points;
 * status (1) int32.  With a non-zero status all three outputs are zero-filled.  At most four launches and two memsets, no host
 * synchronisation; workspace: 256-byte aligned, pn2_frame_sample_workspace_size(cnt) bytes, cleared by the call itself. */
#define PN2_FRAME_MAX_ROWS 16777216
#define PN2_FRAME_ST_OK 0
#define PN2_FRAME_ST_MASK 3
#define PN2_FRAME_ST_CAND 4
int pn2_frame_crop_workspace_size(int n, unsigned long long *bytes);
int pn2_frame_crop(int n, const float *frame, int row_floats, double lo_x, double lo_y, double lo_z, double hi_x, double hi_y,
                   double hi_z, double *out_points, int *out_src, int *out_count, void *workspace, size_t workspace_bytes,
                   void *stream);
int pn2_frame_sample_workspace_size(int cnt, unsigned long long *bytes);
int pn2_frame_sample(int cnt, int npts, const double *points, const unsigned char *mask, double box_size_x, double box_size_y,
                     unsigned long long seed, long long *counter, void *workspace, size_t workspace_bytes, int *out_sel,
                     float *out_centered, double *out_raw, int *status, void *stream);

/* The tiled cover of one scene of the store (csrc/pn2_tile.hip): every point of the scene predicted once per pass, where
 * predict.py's random columns leave coverage to chance.  The scene is cut into the box_size_x x box_size_y columns the network
 * is trained on, every column into as many npts-sized samples as it takes to use each of its points once; each prediction is
 * written back to the point it came from, and passes on shifted grids vote.  The rule (tests/tile_ref.py is its numpy model):
 *
 * pn2_tile_plan: points (n,3) float64, sorted by x ascending as the store keeps them.
 *   grid     ox = points[0,0] - phase_x, oy = min(points[:,1]) - phase_y: the minimum over float64 values, -0.0 the smaller of
 *            two zeros; one float64 subtraction each.  Point p lies in tile (i, j) = (floor((p.x - ox) / box_size_x),
 *            floor((p.y - oy) / box_size_y)): a float64 subtraction, a float64 DIVISION (never a product with a reciprocal),
 *            floor.  A point exactly on a boundary belongs to the upper tile.  phase >= 0 keeps both indices >= 0.
 *   order    (n) int32: the scene positions sorted by (i, j) ascending, equal tiles in ascending position (stable).  A tile is a
 *            maximal run of equal (i, j) in order: its start a, its size m.
 *   samples  (sample_cap,4) int32, rows [a, m, s, S]: a tile with m < min_points has none (its m points are counted as
 *            skipped), any other S = ceil(m / npts) of them, s = 0 .. S-1, listed tile by tile.  Sample s owns the members of
 *            rank r = s (mod S): c = ceil((m - s) / S) <= npts of them.  Row k of [0, npts) of the sample is scene position
 *            order[a + s + (k mod c) * S]; rows k < c are LIVE (the one occurrence of their point in this pass), rows k >= c
 *            the cyclic refill (the doubling loop of semantic_dataset.py:101-106): they feed the network and never vote.  With
 *            min_points = 1 every point of the scene is live in exactly one row of exactly one sample.
 *   header   (8) int32 = [n_tiles, n_samples, skipped_points, status, 0, 0, 0, 0]: n_tiles counts every occupied tile, skipped
 *            ones included; n_samples is the true total even beyond sample_cap (the caller can plan again).
 *   status   0 ok; 1 a NaN or +-inf in an x or y; 2 a tile index outside [0, 2^31); 3 n_samples > sample_cap (rows
 *            [0, sample_cap) are written); the lowest non-zero code wins.  With status 1 or 2 order and samples are written
 *            inside their bounds, but what they hold is not specified.
 * Eight launches, two memsets and a radix sort (hipcub, 64 key bits, stable); every reduction is in integers or ordered keys.  No host
 * synchronisation, no allocation; workspace 256-byte aligned, pn2_tile_plan_workspace_size(n) bytes, cleared by the call, nothing
 * kept between calls.  sample_cap = 0 (samples may be NULL) only counts.
 * PN2_EINVAL: n, npts <= 0, min_points < 1, sample_cap < 0, a box size that is not positive and finite, a phase that is not
 * finite and >= 0, a workspace too small, a misaligned pointer (samples: 16 bytes); PN2_ERANGE: n or npts >
 * PN2_FRAME_MAX_ROWS; PN2_ENULL: points, order, header or workspace NULL, samples NULL with sample_cap > 0.
 *
 * pn2_tile_gather: the batch of the b samples q0 .. q0 + b - 1 of a plan; n_samples and the status are read from the plan's
 * device header, not passed by the host.  For slot i, sample q = q0 + i:
 *   box_min = the float64 minimum over the sample's rows (-0.0 the smaller of two zeros); shift = (min_x + box_size_x / 2,
 *   min_y + box_size_y / 2, min_z) as _center_box (semantic_dataset.py:109-121);
 *   out_data (b,npts,3|6) float32: [k,0:3] = float32(p - shift), the subtraction in float64 and one rounding; [k,3:6] the
 *   float32 colour, copied, with use_color (colors (n,3) float32); out_sel (b,npts) int32 = the scene position of each row;
 *   out_live (b) int32 = c.
 *   A slot with q >= n_samples is a copy of sample n_samples - 1 with live = 0, so the ragged last batch keeps the full batch
 *   shape; with n_samples = 0, or a plan whose status is not 0, every slot is zero-filled with sel = -1 and live = 0.
 * One launch.  PN2_EINVAL: b, npts <= 0, q0 < 0, a bad box size, a misaligned pointer; PN2_ERANGE: npts > PN2_FRAME_MAX_ROWS,
 * b > 65535 or b * npts >= 2^31; PN2_ENULL: a NULL pointer (colors only with use_color).
 *
 * pn2_tile_vote: votes (n,num_class) int32: votes[sel, pred] += 1 for every live row (k < live[q]) of the batch whose prediction
 * lies in [0, num_class); a live row whose prediction does not (or whose sel is negative) is left out and, when dropped != NULL,
 * counted there.  Rows k >= live[q] are ignored.  votes and *dropped accumulate across calls and are never zeroed here.  Integer
 * adds only: the result does not depend on arrival order.  One launch.  PN2_EUNSUP: num_class > 64.
 *
 * pn2_tile_labels: labels[i] = the first maximal class of votes[i, :] (np.argmax); a point without any vote gets 0. */
int pn2_tile_plan_workspace_size(int n, unsigned long long *bytes);
int pn2_tile_plan(int n, const double *points, double box_size_x, double box_size_y, double phase_x, double phase_y, int npts,
                  int min_points, int sample_cap, int *order, int *samples, int *header, void *workspace,
                  size_t workspace_bytes, void *stream);
int pn2_tile_gather(int b, int npts, int q0, int use_color, const double *points, const float *colors, const int *order,
                    const int *samples, const int *header, double box_size_x, double box_size_y, float *out_data, int *out_sel,
                    int *out_live, void *stream);
int pn2_tile_vote(int b, int npts, int num_class, const int *sel, const int *live, const int *pred, int *votes,
                  long long *dropped, void *stream);
int pn2_tile_labels(int n, int num_class, const int *votes, int *labels, void *stream);

/* Soft voting (csrc/pn2_soft_vote.hip, csrc/pn2_label_interp.hip): class probabilities summed over the overlapping predictions
 * of a point and carried to the dense cloud, where pn2_tile_vote and pn2_interpolate_label_with_color count hard labels.
 * tests/soft_vote_ref.py is the numpy model of the four rules.
 *
 * The score format, used by all four: a SCORE ROW is num_class non-negative integers in units of 2^-30, q_c = rint(p_c * 2^30),
 * rounded half to even.  A row of q is int32; accumulated scores are int64.  Integer adds only: sums are exact and independent
 * of the order of arrival, as votes are.  Every entry point checks its arguments in the order of the tile entry points -- sizes
 * (PN2_EINVAL), ranges (PN2_ERANGE), num_class > 64 (PN2_EUNSUP), a required pointer NULL (PN2_ENULL), alignment (PN2_EINVAL) --
 * and refuses before any launch.  No host synchronisation, no allocation: capturable into a graph.
 *
 * pn2_softmax_scores: logits (rows,num_class) float32 -> q (rows,num_class) int32.  Per row, in float64: m = max_c x_c,
 *   e_c = exp((double)x_c - m), s = the sum of e_c added in class order, p_c = e_c / s, q_c = (int)rint(p_c * 2^30).  A row with a
 *   NaN, or with m = +-inf, gets an all-zero score row and is counted in *invalid (optional, accumulates, never zeroed here): such
 *   a row casts no vote downstream.  -inf entries of an otherwise finite row are p = 0.  One launch.
 *
 * pn2_tile_vote_scores: the soft twin of pn2_tile_vote.  scores (n,num_class) int64: for every live row r (k < live[q]) of the
 *   batch with sel[r] >= 0 and all of q[r, :] >= 0, scores[sel[r], c] += q[r, c] for every class.  A live row with sel < 0 or any
 *   negative q is left out whole and counted in *dropped (optional).  Rows k >= live[q] are ignored.  scores and *dropped
 *   accumulate across calls and are never zeroed here.  64-bit integer atomics: duplicated sel within one launch give the exact
 *   sum.  One launch.  PN2_ERANGE: b * npts >= 2^31.
 *
 * pn2_score_labels: labels[i] = the first maximal class of scores[i, :] (an all-zero row gives 0, "unlabeled", like
 *   pn2_tile_labels); confidence[i] (optional, float32) = (float)((double)top / (double)total), total the sum of the row, and 0
 *   when total == 0.  Contract: entries >= 0, row sums below 2^63.  One launch.
 *
 * pn2_interpolate_scores: the soft twin of pn2_interpolate_label_with_color, with its grid, its exact search (float64 squared L2
 *   ((dx*dx + dy*dy) + dz*dz), ascending, ties -> lowest index, min(knn, ns) neighbours), its workspace and its size query
 *   (pn2_interpolate_label_workspace_bytes(ns)); knn <= 16 (PN2_EUNSUP above).  sparse_scores (ns,num_class) int64; contract:
 *   entries >= 0, row sums <= 2^58.  For a dense point S_c = the int64 sum of sparse_scores[j, c] over its neighbours;
 *   dense_labels = the first maximal S_c (all zero -> 0), dense_colors the colour of that label from the table of the label
 *   form, dense_confidence (optional) as in pn2_score_labels.  ns == 0 gives label -1, colour 0, confidence 0.  It queues what
 *   the label form queues: the grid build (its launches, two memsets and a radix sort) and one query launch.  nd == 0 is PN2_OK
 *   whatever the pointers; PN2_EINVAL also for a workspace that is too small. */
int pn2_softmax_scores(int rows, int num_class, const float *logits, int *q, long long *invalid, void *stream);
int pn2_tile_vote_scores(int b, int npts, int num_class, const int *sel, const int *live, const int *q, long long *scores,
                         long long *dropped, void *stream);
int pn2_score_labels(int n, int num_class, const long long *scores, int *labels, float *confidence, void *stream);
int pn2_interpolate_scores(int ns, int nd, int num_class, const float *sparse_points, const long long *sparse_scores,
                           const float *dense_points, int *dense_labels, uint8_t *dense_colors, float *dense_confidence, int knn,
                           void *workspace, size_t workspace_bytes, void *stream);

/* The headless renderer (csrc/pn2_render.hip): a point cloud with per-point colours or labels becomes an image on the device, the
 * counterpart of the reference's Open3D window (visualize.py, colorize.py).  tests/render_ref.py is the numpy model of the rules
 * and is compared for equality: every accumulation is an integer minimum or count, so no result depends on the order of arrival.
 * Every entry point checks its arguments in the order of the tile entry points -- sizes (PN2_EINVAL), ranges (PN2_ERANGE),
 * unsupported (PN2_EUNSUP), a required pointer NULL (PN2_ENULL), alignment (PN2_EINVAL) -- and refuses before any launch.  No
 * host synchronisation, no allocation: capturable into a graph.  One launch each.
 *
 * pn2_label_colors: util/point_cloud_util.py:_label_to_colors.  labels (n) int32, palette (num_class,3) uint8 in device memory,
 *   colors (n,3) uint8 = palette[labels].  A label outside [0, num_class) gives 0,0,0 and is counted in *bad (optional int64,
 *   accumulates, never zeroed here) where the reference raises.  PN2_EUNSUP: num_class > 256.
 *
 * pn2_render_splat: points (n,3) float32, or float64 with points_f64 = 1.  view: a HOST pointer to 12 doubles, the row-major 3x4
 *   matrix M, copied by value into the launch (frozen at capture).  zbuf (height*width) uint64, 8-byte aligned, accumulates across
 *   calls; "empty" is all bits set (the caller clears it with a 0xFF fill).  For point i = (x, y, z), in float64 without
 *   contraction:
 *     t_r  = ((M[r][0]*x + M[r][1]*y) + M[r][2]*z) + M[r][3]
 *     perspective = 0: u = t_0, v = t_1, d = t_2;  perspective = 1: d = t_2, u = t_0 / d, v = t_1 / d, culled when !(d > 0).
 *     culled unless u, v and d are finite and -2^30 <= u, v < 2^30 (tested in floating point before any conversion to int).
 *     px = (int)floor(u), py = (int)floor(v); the point covers the pixels (px - size/2 + a, py - size/2 + b), 0 <= a, b < size
 *     (integer division), each kept iff it lies inside the image; a point that keeps none counts as culled.  *culled
 *     (optional int64, accumulates) gets one count per culled point.
 *     f = (float)d + 0.0f (to nearest; -0 becomes +0); k = the order-preserving uint32 image of f (every bit of a negative f
 *     flipped, the sign bit of a non-negative f set); key = ((uint64)k << 32) | (uint32)(index0 + i);
 *     zbuf[py*width + px] = min(zbuf[py*width + px], key), a 64-bit unsigned atomic minimum.
 *   The nearest depth wins, equal float32 depths go to the lowest global index; the result is the same for any order of points,
 *   any chunking and any order of calls.  PN2_EINVAL: n, width, height or size <= 0, a flag that is neither 0 nor 1;
 *   PN2_ERANGE: index0 < 0, index0 + n > 2^31 - 1, width * height >= 2^31; PN2_EUNSUP: size > 16.
 *
 * pn2_render_resolve: per pixel p of zbuf: index[p] (optional int32) = the low word of the key, -1 where empty; depth[p] (optional
 *   float32) = f recovered from k, +inf where empty; image[p] (optional, (height,width,3) uint8) = colors[index] of colors
 *   (npoints,3) uint8, the 3 HOST bytes background (copied by value) where the pixel is empty or its index >= npoints (never read
 *   out of bounds).  PN2_ENULL: zbuf NULL, all three outputs NULL, image without background or without colors (npoints > 0). */
int pn2_label_colors(int n, int num_class, const int *labels, const uint8_t *palette, uint8_t *colors, long long *bad,
                     void *stream);
int pn2_render_splat(int n, int index0, const void *points, int points_f64, const double *view, int perspective, int width,
                     int height, int size, unsigned long long *zbuf, long long *culled, void *stream);
int pn2_render_resolve(int width, int height, const unsigned long long *zbuf, int npoints, const uint8_t *colors,
                       const uint8_t *background, uint8_t *image, float *depth, int *index, void *stream);

/* Euclidean clustering (csrc/pn2_cluster.hip): the points of a cloud, optionally of one label each, grouped into objects.
 * tests/cluster_ref.py is the numpy model of the rules and is compared for equality: nothing in a result depends on the order in
 * which threads arrive.
 *
 *   points (n,3) float32; labels (n) int32 or NULL (one class); eps finite and > 0; min_points >= 1; max_points >= 0 (0: no upper
 *   bound).
 *   A point is VALID when its three coordinates are finite and, with labels, its label is >= 0.
 *   Two valid points i != j are LINKED when their labels are equal (with labels) and, in float64 without contraction,
 *     (dx*dx + dy*dy) + dz*dz <= (double)eps * (double)eps,   dx = (double)x_i - (double)x_j, dy and dz likewise.
 *   A COMPONENT is a connected component of that graph; its first = its lowest point index, its size = its point count.  It is
 *   KEPT when min_points <= size and (max_points == 0 or size <= max_points).  The kept components are numbered 0 .. C-1 by
 *   ascending first.  ids[i] = the number of the component of i; -1 for an invalid point and for a point of a component that is
 *   not kept.
 *
 * pn2_cluster_points: ids (n) int32 and header (8) int32 on the device: [0] status, [1] C, [2] components before the size filter,
 *   [3] valid points, [4] points in kept clusters, [5..7] zero.  Status 0 = ok; 1 = more than 2^21 cells of edge eps on an axis
 *   of the valid points' box (the convention of pn2_voxel_downsample): then every id is -1 and header[1..7] are zero.
 *   workspace: *bytes of pn2_cluster_workspace_size(n, bytes) (a host query like pn2_tile_plan_workspace_size: PN2_EINVAL for
 *   n <= 0, PN2_ENULL without bytes), 256-byte aligned.  It queues a sorted-key grid build (its
 *   launches and a radix sort), a lock-free union-find over the 27 cells around every point, and an ordered numbering; no
 *   allocation, no synchronisation.  It is eager by nature -- the caller reads C from the header before it can size what follows
 *   -- and refuses a capturing stream: PN2_EUNSUP, before anything is launched.  Checked before that, in this order, nothing
 *   launched: PN2_EINVAL (n <= 0, eps not finite or <= 0, min_points < 1, max_points < 0), PN2_ENULL (points, ids, header or
 *   workspace NULL), PN2_EINVAL (a misaligned pointer, a workspace that is too small).
 *
 * pn2_cluster_stats: per cluster c of ids (as written by pn2_cluster_points; nclusters = C >= 1): first[c] = its lowest point
 *   index, size[c] = its point count, label[c] = labels[first[c]] (0 without labels), bbox (nclusters,6) float32 = min x, y, z
 *   then max x, y, z: exact minima and maxima of the members' float32 coordinates (-0.0 below +0.0).  Integer atomics only.  An id
 *   outside [0, nclusters) is ignored; a cluster without points keeps first = 2^31 - 1, size 0, label 0 and a box of NaNs.
 *   Three launches.  PN2_EINVAL: n or nclusters <= 0, a misaligned pointer; PN2_ERANGE: nclusters > n; PN2_ENULL: any pointer but
 *   labels NULL.
 *
 * pn2_cluster_colors: rgb (n,3) uint8, one colour of full saturation per id: in uint32 arithmetic
 *     h = id * 0x9E3779B1;  h ^= h >> 15;  h *= 0x85EBCA77;  h ^= h >> 13;  hue = h % 1536;  s = hue >> 8;  f = hue & 255;
 *     (r,g,b) = (255,f,0), (255-f,255,0), (0,255,f), (0,255-f,255), (f,0,255), (255,0,255-f)  for s = 0 .. 5.
 *   A negative id gives (96,96,96).  One launch. */
int pn2_cluster_workspace_size(int n, unsigned long long *bytes);
int pn2_cluster_points(int n, const float *points, const int *labels, float eps, int min_points, int max_points, int *ids,
                       int *header, void *workspace, size_t workspace_bytes, void *stream);
int pn2_cluster_stats(int n, int nclusters, const float *points, const int *labels, const int *ids, int *first, int *size,
                      int *label, float *bbox, void *stream);
int pn2_cluster_colors(int n, const int *ids, uint8_t *rgb, void *stream);

/* Object description (csrc/pn2_describe.hip): per cluster its member count, centroid, principal axes, variances and the oriented
 * box around its members (what Open3D calls get_oriented_bounding_box), and the boxes drawn as points.  tests/describe_ref.py is
 * the numpy model of the rules and is compared for equality: every accumulation is an integer sum or an integer minimum / maximum,
 * and everything else is float64 in the written association (the library is built without contraction; sqrt and / are correctly
 * rounded), so nothing in a result depends on the order in which threads arrive.
 *
 *   points (n,3) float32; ids (n) int32.  Point i is a MEMBER of cluster c when ids[i] == c, 0 <= c < nclusters, and its three
 *   coordinates are finite.  Every other point is ignored.  pn2_cluster_describe computes its own box from the members: it does
 *   not depend on pn2_cluster_stats.
 *
 * Per cluster with m >= 1 members:
 *   BOX AND LATTICE.  o = the per-axis minimum of the members' coordinates, widened to float64.  E = the maximum over the axes
 *     of (double)max - (double)min.  Q = min(20, (62 - bitlen(m)) >> 1), bitlen = the number of bits of m.  If E > 0:
 *     E = f * 2^x with f in [0.5, 1) (frexp) and h = 2^(x-Q); if E == 0: x = Q, h = 1.  Per member and axis
 *     q = (long long)rint(((double)p - o) / h), ties to even; the division is exact (h is a power of two); 0 <= q <= 2^Q.
 *   MOMENTS (int64).  S_a = sum q_a, S_ab = sum q_a * q_b for ab in xx, xy, xz, yy, yz, zz; by the choice of Q every sum is below
 *     2^62.  Integer adds only.
 *   CENTROID.  centroid_a = o_a + ((double)S_a / (double)m) * h.
 *   COVARIANCE in lattice units.  A_ab = (double)S_ab / (double)m - ((double)S_a / (double)m) * ((double)S_b / (double)m).
 *   AXES, upright = 0.  Eight cyclic Jacobi sweeps over the pairs (p,r) = (0,1), (0,2), (1,2), k the third index, V = identity at
 *     the start.  A pair with A_pr == 0 is skipped.  Otherwise
 *       theta = (A_rr - A_pp) / (2 * A_pr);  t = sigma / (|theta| + sqrt(theta * theta + 1)), sigma = +1 if theta >= 0 else -1;
 *       c = 1 / sqrt(t * t + 1);  s = t * c;
 *       A_pp -= t * A_pr;  A_rr += t * A_pr;  A_pr = 0;
 *       A_kp' = c * A_kp - s * A_kr;  A_kr' = s * A_kp + c * A_kr;
 *       for each row i of V:  V_ip' = c * V_ip - s * V_ir;  V_ir' = s * V_ip + c * V_ir.
 *     (A theta * theta that overflows gives t = +-0 by IEEE rules: intended.)  The eigenpairs (diagonal entry, column of V) are
 *     sorted by descending diagonal, equal values keep the lower column first.  a0 and a1 are the first two columns, each negated
 *     if its component of largest magnitude (the first among equals) is negative.  a2 = a0 x a1, each component as u*v - w*z.
 *   AXES, upright = 1.  The same single rotation on the pair (0,1) only; the two in-plane eigenpairs sorted the same way; a0 takes
 *     the sign rule; a1 = (-a0_y, a0_x, 0); a2 = (0,0,1); lambda_2 = A_zz.
 *   VARIANCES.  variance_k = lambda_k * (h * h).
 *   EXTENTS (a second pass over the points).  Per member d = (double)p - centroid and t_k = (a_k0 * d_x + a_k1 * d_y) + a_k2 * d_z;
 *     lo_k, hi_k = the minimum and maximum over the members, taken as unsigned 64-bit atomic min / max on the order-preserving
 *     image of the double (-0.0 sorts below +0.0).
 *   BOX CENTRE.  center_a = centroid_a + ((a_0a * g_0 + a_1a * g_1) + a_2a * g_2), g_k = 0.5 * (lo_k + hi_k).
 *
 * pn2_cluster_describe: moments (nclusters,12) int64: [0] m, [1..3] S_x S_y S_z, [4..9] S_xx S_xy S_xz S_yy S_yz S_zz, [10] Q,
 *   [11] x; desc (nclusters,24) float64: [0..2] centroid, [3..5] variances, [6..14] a0, a1, a2, [15..17] lo, [18..20] hi, [21..23]
 *   box centre.  A cluster without members gets a zero moments row and a desc row of NaNs.
 *   workspace: *bytes of pn2_cluster_describe_workspace_size(nclusters, bytes) (a host query like pn2_cluster_workspace_size:
 *   PN2_EINVAL for nclusters <= 0, PN2_ENULL without bytes), 256-byte aligned; it need not be cleared.  Seven launches: three
 *   passes over the points (box and count, moments, extents), each of which reduces inside the wave before it issues an atomic,
 *   and one thread per cluster in between.  No allocation, no host read, no synchronisation.
 *   Refusals, nothing launched, in this order: PN2_EINVAL (n or nclusters <= 0, upright not 0 or 1), PN2_ERANGE (nclusters > n),
 *   PN2_ENULL (any pointer NULL), PN2_EINVAL (points or ids not 4-byte aligned, moments or desc not 8-byte aligned, a workspace
 *   not 256-byte aligned or too small), PN2_EUNSUP (a capturing stream: it would be capturable, but nothing in the project
 *   captures it yet, so the refusal stands until a later change lifts it together with a capture test).
 *
 * pn2_box_wireframe: the 12 edges of every box of desc as per_edge points each: points (nclusters*12*per_edge, 3) float32, owner
 *   (nclusters*12*per_edge) int32 = the cluster index, in the order cluster, edge, sample.  Corner j (bits j0 j1 j2) is
 *   centroid + ((a_0 * e_0 + a_1 * e_1) + a_2 * e_2), e_k = hi_k if bit k of j is set, else lo_k.  The edges join corners that
 *   differ in one bit: for k = 0, 1, 2 and for the four values of the other two bits in ascending order, from the corner A without
 *   bit k to the corner B with it.  Sample s is A + (B - A) * ((double)s / (double)(per_edge - 1)), rounded to float32.  A row of
 *   NaNs gives NaN points, which the renderer culls.  One launch, capturable.  PN2_EINVAL: nclusters <= 0, per_edge < 2;
 *   PN2_ERANGE: nclusters * 12 * per_edge >= 2^31; PN2_ENULL: a NULL pointer; PN2_EINVAL: desc not 8-byte, points or owner not
 *   4-byte aligned. */
int pn2_cluster_describe_workspace_size(int nclusters, unsigned long long *bytes);
int pn2_cluster_describe(int n, int nclusters, const float *points, const int *ids, int upright, long long *moments, double *desc,
                         void *workspace, size_t workspace_bytes, void *stream);
int pn2_box_wireframe(int nclusters, const double *desc, int per_edge, float *points, int *owner, void *stream);

/* Plane segmentation (csrc/pn2_plane.hip): the dominant plane of a cloud by random sample consensus (RANSAC) -- the ground of a
 * LiDAR frame, a road, a floor, a facade.  tests/plane_ref.py is the numpy model of the rules and is compared for equality: the
 * decisions are float64 comparisons in a fixed order (the library is built without contraction) and everything after them is
 * integer, so nothing in a result depends on the order in which threads arrive.  No square root and no division anywhere.
 *
 *   points (n,3) float32; labels (n) int32 or NULL.  A point is VALID when its three coordinates are finite and, with labels, its
 *   label is >= 0 (the rule of pn2_cluster_points).
 *   A PLANE is six doubles (x0,y0,z0, a,b,c): a point on it and an unnormalised normal.  nn = (a*a + b*b) + c*c.  The plane is
 *   VOID when nn is not finite or not > 0.
 *   A point p is an INLIER of a non-void plane when, with e = (a*(x-x0) + b*(y-y0)) + c*(z-z0) in float64 (x the float32
 *   coordinate widened), the comparison  e*e <= thr2*nn  is true, thr2 = (double)thr * (double)thr, thr float32, finite and > 0.
 *   A NaN on either side makes the comparison false, and so does an e*e that overflows against a finite thr2*nn.
 *   AXIS CONSTRAINT (optional): axis (3) float64 ON THE HOST or NULL, cos2 in [0,1].  A non-void plane is additionally void when
 *     dt*dt >= (cos2*nn) * ((ax*ax + ay*ay) + az*az),  dt = (a*ax + b*ay) + c*az,  is false: its normal is further from the axis
 *   (or its opposite) than the angle whose squared cosine is cos2.
 *
 * pn2_plane_score: counts[t] = the number of valid inliers of plane t of planes (nplanes,6) float64, 0 for a void plane; counts
 *   (nplanes) int32.  Public in its own right: it scores hypotheses carried over from an earlier frame.  Two launches: one that
 *   clears counts (no memset node), one in which a lane owns a plane and a workgroup 256 planes and chunks of 1024 points staged
 *   in LDS as doubles; every lane adds its partial count with one integer atomicAdd.  PN2_EINVAL: n < 1, nplanes outside
 *   [1, 2^24], thr not finite or <= 0; PN2_ENULL: points, planes or counts NULL; PN2_EINVAL: points, labels, counts not 4-byte
 *   or planes not 8-byte aligned; PN2_EUNSUP: a capturing stream (below).
 *
 * pn2_plane_workspace_size: *bytes = the workspace of pn2_plane_ransac(n, trials) (a host query like pn2_cluster_workspace_size:
 *   PN2_EINVAL for n < 1 or trials outside [1, 2^20], PN2_ENULL without bytes).
 *
 * pn2_plane_ransac queues, with no allocation and no synchronisation:
 *   1 the valid point indices in ascending order (an ordered compaction); V = their number.
 *   2 the hypotheses t = 0 .. trials-1: with h = sample_stream(seed, 0, 0) of csrc/pn2_rng.h, the sample points A, B, C are the
 *     valid points of rank draw64(h, 2^45 + 3t + j) % V, j = 0, 1, 2 (unsigned 64-bit); as doubles, u = B-A, v = C-A, the normal
 *     is (uy*vz - uz*vy, uz*vx - ux*vz, ux*vy - uy*vx) and the origin A.  Repeated ranks and collinear points give nn == 0: void.
 *     With an axis, the planes it excludes are void too.
 *   3 the scores of pn2_plane_score (a void trial scores 0; a non-void one at least 1: its origin is a valid point with e == 0).
 *   4 the winner: the largest count, the lowest t among equal counts.
 *   5 inlier (n) uint8: 1 for the valid inliers of the winner, 0 for every other point;
 *     plane (4) float64 = the raw (a,b,c,d), d = -((a*x0 + b*y0) + c*z0), oriented by negating all four exactly: with an axis so
 *     that dt >= 0, without one so that the first non-zero of (c,b,a) is positive.  Not normalised: it stays comparable for
 *     equality.
 *   6 header (8) int32: [0] status, [1] inlier count, [2] winning trial, [3..5] the point indices of A, B, C, [6] V, [7] the
 *     number of non-void trials.  Status 0 = ok; 1 = V < 3; 2 = every trial void.  With a status other than 0, inlier is all 0,
 *     plane is four zeros and header[1..5] = 0, 0, -1, -1, -1.
 *   workspace: 256-byte aligned, at least pn2_plane_workspace_size bytes.  Refusals, nothing launched and nothing written, in this
 *   order: PN2_EINVAL (n < 1, trials outside [1, 2^20], thr not finite or <= 0, with an axis: cos2 outside [0,1] or NaN, an axis
 *   that is non-finite or all zero), PN2_ENULL (points, inlier, plane, header or workspace NULL), PN2_EINVAL (points, labels,
 *   header not 4-byte or plane not 8-byte aligned, workspace not 256-byte aligned or too small), PN2_EUNSUP (a capturing stream).
 *
 * Both pn2_plane_score and pn2_plane_ransac refuse a capturing stream.  They allocate nothing and would be capturable; nothing in
 * the project captures them yet, so the refusal stands until a later change lifts it together with a capture test. */
int pn2_plane_score(int n, const float *points, const int *labels, int nplanes, const double *planes, float thr, int *counts,
                    void *stream);
int pn2_plane_workspace_size(int n, int trials, unsigned long long *bytes);
int pn2_plane_ransac(int n, const float *points, const int *labels, float thr, int trials, unsigned long long seed,
                     const double *axis, double cos2, unsigned char *inlier, double *plane, int *header, void *workspace,
                     size_t workspace_bytes, void *stream);

/* Fixed-radius neighbourhoods (csrc/pn2_neighbors.hip): per point the number of points within `radius` of it, the integer moments
 * of that neighbourhood, the surface normal and the surface variation there -- what Open3D offers as estimate_normals with
 * KDTreeSearchParamRadius and as remove_radius_outlier.  tests/neighbors_ref.py is the numpy model of the rules and is compared
 * for equality: a neighbourhood is decided by a float64 comparison, its sums are integer adds, and everything after them is
 * float64 in the written association (no contraction; sqrt and / correctly rounded), so nothing in a result depends on the order
 * in which threads arrive or on which candidates a thread looks at.
 *
 *   points (n,3) float32; labels (n) int32 or NULL; radius float32, finite and > 0; min_neighbors >= 1; viewpoint (3) float64 ON
 *   THE HOST (read before the call returns) or NULL.
 *   VALID.  The rule of pn2_cluster_points: three finite coordinates and, with labels, a label >= 0.
 *   NEIGHBOUR.  For a valid point i every valid point j, i ITSELF INCLUDED (labels need not be equal), with, in float64,
 *       (dx*dx + dy*dy) + dz*dz <= r*r,   r = (double)radius,   dx = (double)x_j - (double)x_i (exact), dy and dz likewise.
 *     count[i] = the number of neighbours, at least 1 for a valid point; 0 for an invalid one.
 *   LATTICE, one per call.  Q = min(20, (60 - bitlen(n)) >> 1), bitlen = the number of bits of n.  r = f * 2^x with f in [0.5, 1)
 *     (frexp) and h = 2^(x-Q).  Per neighbour and axis q = (long long)rint(d / h), ties to even, d the difference above.  The
 *     division is exact (h is a power of two), and |q| <= 2^Q: the test bounds |d| by r * (1 + 2^-51), and r <= (1 - 2^-24) * 2^x.
 *   MOMENTS (int64).  S_x S_y S_z S_xx S_xy S_xz S_yy S_yz S_zz = the sums of q_a and of q_a * q_b over the neighbours.  Every sum
 *     is at most n * 2^(2Q) <= 2^60 in magnitude.  Integer adds only, so no order of arrival shows.
 *   COVARIANCE AND AXES.  Exactly the rules of pn2_cluster_describe with m = count and upright = 0:
 *     A_ab = (double)S_ab / (double)m - ((double)S_a / (double)m) * ((double)S_b / (double)m); eight cyclic Jacobi sweeps; the
 *     eigenpairs sorted by descending diagonal, equal values keeping the lower column first; a0 and a1 sign-fixed; a2 = a0 x a1.
 *   NORMAL.  It starts from a2, negated when its component of largest magnitude (the first among equals) is negative.  With a
 *     viewpoint v:  w = ((v_x - p_x) * n_x + (v_y - p_y) * n_y) + (v_z - p_z) * n_z  in float64, p the point widened; the normal
 *     is negated when w < 0.  A zero or NaN w changes nothing.  The output is float32, each component rounded once.
 *   CURVATURE (surface variation).  t = (lambda_0 + lambda_1) + lambda_2;  c = lambda_2 / t;  c = 0 unless c > 0 (so 0 / 0 and a
 *     negative rounding residue give 0).  The output is float32.
 *   VARIANCE.  variance_k = lambda_k * (h * h), float64.
 *   POINTS WITHOUT A RESULT.  A valid point with count < min_neighbors keeps its count and its moments; its normal, curvature and
 *     variance are NaN.  An invalid point has count 0, a zero moments row and NaNs.
 *
 * pn2_radius_neighborhoods: count (n) int32; moments (n,9) int64 or NULL; normals (n,3) float32; curvature (n) float32; variance
 *   (n,3) float64 or NULL; header (8) int32 on the device: [0] status, [1] valid points, [2] points with count >= min_neighbors,
 *   [3] the largest count, [4] Q, [5] x, [6..7] zero.  Status 0 = ok; 1 = more than 2^21 cells of edge radius on an axis of the
 *   valid points' box (the convention of pn2_cluster_points): then every count is 0, the moments are zero, normals, curvature and
 *   variance are NaN and header[1..7] are zero.  moments and variance are written only when given; the other outputs are the
 *   same bits either way.
 *   workspace: *bytes of pn2_radius_workspace_size(n, bytes) (a host query like pn2_cluster_workspace_size: PN2_EINVAL for
 *   n <= 0, PN2_ENULL without bytes), 256-byte aligned; it need not be cleared.  The call queues the sorted-key grid of
 *   pn2_cluster_points (cell edge radius * (1 + 2^-20), its launches and one radix sort) and one scan in which a lane owns a
 *   point and keeps its count and sums in registers: no atomic on a sum, no memset node, no allocation, no synchronisation.
 *   Refusals, nothing launched and nothing written, in this order: PN2_EINVAL (n < 1, radius not finite or <= 0, min_neighbors
 *   < 1, a non-finite viewpoint), PN2_ENULL (points, count, normals, curvature, header or workspace NULL), PN2_EINVAL (points,
 *   labels, count, normals, curvature or header not 4-byte aligned, moments or variance not 8-byte aligned, a workspace not
 *   256-byte aligned or too small), PN2_EUNSUP (a capturing stream: it allocates nothing and would be capturable, but nothing in
 *   the project captures it, so the refusal stands until a later change lifts it together with a capture test). */
int pn2_radius_workspace_size(int n, unsigned long long *bytes);
int pn2_radius_neighborhoods(int n, const float *points, const int *labels, float radius, int min_neighbors,
                             const double *viewpoint, int *count, long long *moments, float *normals, float *curvature,
                             double *variance, int *header, void *workspace, size_t workspace_bytes, void *stream);

/* Rigid registration (ICP) (csrc/pn2_icp.hip): the rigid motion that lays a SOURCE cloud onto a TARGET cloud by iterative closest
 * point -- what Open3D offers as registration_icp (TransformationEstimationPointToPoint / PointToPlane), evaluate_registration
 * and PointCloud.transform.  tests/icp_ref.py is the numpy model of the rules and is compared for equality.  A partner is decided
 * by float64 comparisons; everything after the sums is float64 in the written association (no contraction; sqrt and / correctly
 * rounded).  THE SUMS ARE FLOAT64 TOO, and here this section departs from its siblings' integer sums: the point-to-plane products
 * are squares of (coordinate x normal component) terms, which do not fit 2^62 on any lattice fine enough to be useful.  They are
 * added in ONE FIXED TREE over the source index instead (SUMS), so a result is the same on every run and for every order in
 * which threads arrive -- but it is a function of the ORDER of the source points: a permuted source gives the same partners and,
 * in its last bits, another transformation.
 *
 *   source (ns,3), target (nt,3) float32; source_labels (ns), target_labels (nt) int32 or NULL; target_normals (nt,3) float32,
 *   needed for estimation 1; max_distance float32, finite and > 0; init: 16 doubles, row-major 4x4, ON THE HOST (read before the
 *   call returns), or NULL = the identity; max_iteration >= 0; relative_fitness, relative_rmse >= 0.
 *   VALID.  The rule of pn2_cluster_points: three finite coordinates and, with labels, a label >= 0.  With estimation 1 a target
 *     point also needs three finite normal components.
 *   TRANSFORMED SOURCE POINT.  With T the current 4x4 (float64) and (x, y, z) the float32 point widened, per axis a = 0, 1, 2
 *       s'_a = (float)(((T_a0*x + T_a1*y) + T_a2*z) + T_a3):  float64 without contraction, rounded to float32 once.
 *     Row 3 of T is carried along and never read.  A source point with a non-finite s' has no partner.
 *   PARTNER.  Of a valid source point: the valid target point with the smallest d2 = (dx*dx + dy*dy) + dz*dz in float64,
 *     dx = (double)t_x - (double)s'_x, dy and dz likewise, among those with d2 <= r*r, r = (double)max_distance; equal d2 go to
 *     the lowest target index.  correspondence[i] = that index; -1 without a partner and for an invalid source point.
 *   GRID.  The target's, built once per call: the minimum, keys and one radix sort of csrc/pn2_cell_grid.h at cell edge
 *     h = r * (1 + 2^-20).  o = the per-axis minimum of the valid target points, widened to float64 (-0.0 below +0.0).  The
 *     cell of a source point is c_a = floor(((double)s'_a - o_a) / h), against the TARGET's minimum, so it may be negative.  A
 *     point with c_a < -1 or c_a > 2^21 on an axis (decided in floating point before any conversion; a NaN quotient -- no valid
 *     target point -- likewise) has no partner; otherwise the cells c-1 .. c+1 clipped to [0, 2^21) are searched, as nine key
 *     ranges.  Why that finds every partner: pn2_cell_grid.h's proof bounds the error of a computed quotient by 2^-31 from
 *     |a/h| < 2^21 alone, not from a >= 0; here |a/h| <= 2^21 + 1, the bound doubles at the most, and with it
 *     q_i - q_j < 1 - 2^-21 + 2^-29 < 1 still holds for a pair that passes the distance test, whatever the signs -- and two
 *     numbers less than 1 apart have floors at most 1 apart.  So a source point whose floor is below -1 or above 2^21 would need
 *     a partner with a floor below 0 or of 2^21 and more, and no valid target point of a status-0 call has one.
 *   SUMS.  Float64.  Source point i is lane i % 64 of wave (i / 64) % 4 of workgroup i / 256; the source is not sorted.  A lane
 *     without a partner (and a lane beyond ns) contributes +0.0 to every sum.  Per sum: inside the wave v = v + v[lane ^ o] for
 *     o = 32, 16, 8, 4, 2, 1 (every lane ends with the same value); the workgroup's value is ((w0 + w1) + w2) + w3; the
 *     call's value is 0.0 + g_0 + g_1 + ..., the workgroups added in ascending order.  Coordinates enter relative to o:
 *     p_a = (double)s'_a - o_a and u_a = (double)t_a - o_a for the partner t.
 *   EVALUATION k (k = 0, 1, ...) matches under T_k (T_0 = init) and gives m_k = the number of pairs (a sum of 1.0s),
 *     D_k = the sum of d2, fitness_k = m_k / (the number of valid source points), 0 when there is none, and
 *     rmse_k = sqrt(D_k / m_k), 0 when m_k == 0.
 *   STOP after evaluation k, the first that applies:  the status is 1 (GRID, below);  k >= 1 and |fitness_k - fitness_(k-1)| <
 *     relative_fitness and |rmse_k - rmse_(k-1)| < relative_rmse (Open3D's test: absolute differences despite the names; it sets
 *     "converged");  k == max_iteration;  the update cannot be formed: status 2, T stays T_k.  Otherwise T_(k+1) = U_k * T_k:
 *     row a < 3, column b:  ((R_a0*T_0b + R_a1*T_1b) + R_a2*T_2b) + t_a*T_3b;  row 3 is kept.  max_iteration = 0 evaluates init
 *     and changes nothing (evaluate_registration).
 *   POINT-TO-POINT (estimation 0).  Sums: m, D, P_a = sum p_a, U_a = sum u_a, C_ab = sum p_a * u_b.  m < 3: status 2.
 *     pm_a = P_a / m, um_a = U_a / m, M_ab = C_ab / m - pm_a * um_b.  Horn's symmetric 4x4:
 *       N00 = (Mxx + Myy) + Mzz   N11 = (Mxx - Myy) - Mzz   N22 = (Myy - Mxx) - Mzz   N33 = (Mzz - Mxx) - Myy
 *       N01 = Myz - Mzy   N02 = Mzx - Mxz   N03 = Mxy - Myx   N12 = Mxy + Myx   N13 = Mzx + Mxz   N23 = Myz + Mzy.
 *     It is diagonalised by ten cyclic Jacobi sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) from V = identity, each
 *     rotation that of pn2_cluster_describe (AXES) with its "third index" step applied to both other indices k.  The quaternion
 *     (w, x, y, z) is the column of V under the largest diagonal entry, the first among equals.  ROTATION OF A QUATERNION:
 *       nn = ((w*w + x*x) + y*y) + z*z
 *       R00 = (((w*w + x*x) - y*y) - z*z) / nn   R01 = (2 * (x*y - w*z)) / nn             R02 = (2 * (x*z + w*y)) / nn
 *       R10 = (2 * (x*y + w*z)) / nn             R11 = (((w*w - x*x) + y*y) - z*z) / nn   R12 = (2 * (y*z - w*x)) / nn
 *       R20 = (2 * (x*z - w*y)) / nn             R21 = (2 * (y*z + w*x)) / nn             R22 = (((w*w - x*x) - y*y) + z*z) / nn
 *     (no trigonometry anywhere).  t_a = (um_a + o_a) - ((R_a0*c_0 + R_a1*c_1) + R_a2*c_2), c_a = pm_a + o_a.
 *   POINT-TO-PLANE (estimation 1).  Per pair, n = the partner's normal widened: e_a = (double)s'_a - (double)t_a,
 *     rho = (e_x*n_x + e_y*n_y) + e_z*n_z, J = (p_y*n_z - p_z*n_y, p_z*n_x - p_x*n_z, p_x*n_y - p_y*n_x, n_x, n_y, n_z).  Sums: m,
 *     D, the 21 products J_a * J_b (a <= b) = A, the 6 products J_a * rho = g.  m < 6: status 2.  A = L * L^T by Cholesky, for
 *     j = 0 .. 5:  d = A_jj, then d -= L_jk * L_jk for k = 0 .. j-1;  a d that is not > 0: status 2;  L_jj = sqrt(d);  for
 *     i = j+1 .. 5:  v = A_ij, then v -= L_ik * L_jk for k = 0 .. j-1;  L_ij = v / L_jj.  Forward, i = 0 .. 5:  v = -g_i, then
 *     v -= L_ik * y_k for k = 0 .. i-1;  y_i = v / L_ii.  Backward, i = 5 .. 0:  v = y_i, then v -= L_ki * x_k for
 *     k = i+1 .. 5;  x_i = v / L_ii.  R = the rotation of the quaternion (1, x_0 / 2, x_1 / 2, x_2 / 2);
 *     t_a = (o_a + x_(3+a)) - ((R_a0*o_0 + R_a1*o_1) + R_a2*o_2).
 *
 * pn2_icp: correspondence (ns) int32 = that of the last evaluation; result (20) float64: [0..15] the final T, [16] fitness,
 *   [17] inlier rmse, [18] D of the last evaluation, [19] 0; header (8) int32: [0] status, [1] valid source points, [2] valid
 *   target points, [3] m of the last evaluation, [4] updates applied (= the index of the last evaluation), [5] 1 when the
 *   criterion stopped it, [6..7] 0; trace (max_iteration + 1, 20) float64 or NULL: row k = [0] m_k, [1] fitness_k, [2] rmse_k,
 *   [3] 0, [4..19] T_k; the rows behind the last evaluation are zero.  All on the device.  The other outputs are the same bits
 *   with and without a trace.  Status 0 = ok; 1 = more than 2^21 cells of edge max_distance on an axis of the valid target
 *   points' box (the convention of pn2_cluster_points): then every correspondence is -1, result = init followed by four zeros,
 *   header[1..7] are zero and trace row 0 is (0, 0, 0, 0, init); 2 = too few pairs or a pivot that is not positive.
 *   workspace: *bytes of pn2_icp_workspace_size(ns, nt, max_iteration, bytes) (a host query like pn2_cluster_workspace_size:
 *   PN2_EINVAL for ns or nt < 1 or max_iteration < 0, PN2_ENULL without bytes; it does not decrease when an argument grows),
 *   256-byte aligned; it need not be cleared.  The call queues an init kernel (the scalars, the trace zeroed: no memset node), the
 *   target's grid, and max_iteration + 1 pairs of launches: icp_match_kernel, in which a lane owns a source point -- transform,
 *   search, its row of the sums in registers, the tree; no atomic on a sum, one row of partials per workgroup in the workspace
 *   -- and the one-workgroup icp_step_kernel, which adds the rows, decides and updates T.  The whole loop runs without the host:
 *   the step that stops sets a `done` word, and every later launch reads it and returns without writing anything.  No
 *   allocation, no synchronisation, no dynamic-LDS limit raised.
 *   Refusals, nothing launched and nothing written, in this order: PN2_EINVAL (ns or nt < 1, max_distance not finite or <= 0,
 *   estimation not 0 or 1, max_iteration < 0, a tolerance that is NaN or negative, a non-finite init), PN2_ENULL (source,
 *   target, correspondence, result, header or workspace NULL; target_normals NULL with estimation 1), PN2_EINVAL (source,
 *   target, the labels, target_normals, correspondence or header not 4-byte aligned, result or trace not 8-byte aligned, a
 *   workspace not 256-byte aligned or too small), PN2_EUNSUP (a capturing stream: the loop's length is data, a capture would
 *   record every round).
 *
 * pn2_transform_points: out (n,3) float32 = the TRANSFORMED SOURCE POINT of every row of points under transform (16 doubles on
 *   the HOST, copied by value); a row with a non-finite coordinate is copied as it is.  out may be points.  One launch,
 *   capturable.  PN2_EINVAL: n < 1; PN2_ENULL: a NULL pointer; PN2_EINVAL: a non-finite transform, points or out not 4-byte
 *   aligned. */
int pn2_icp_workspace_size(int ns, int nt, int max_iteration, unsigned long long *bytes);
int pn2_icp(int ns, const float *source, const int *source_labels,
            int nt, const float *target, const int *target_labels, const float *target_normals,
            float max_distance, int estimation /* 0 point-to-point, 1 point-to-plane */,
            const double *init /* 16, row-major, ON THE HOST, or NULL = identity */,
            int max_iteration, double relative_fitness, double relative_rmse,
            int *correspondence /* (ns) */, double *result /* (20) */, double *trace /* (max_iteration+1, 20) or NULL */,
            int *header /* (8) */, void *workspace, size_t workspace_bytes, void *stream);
int pn2_transform_points(int n, const float *points, const double *transform /* 16, host */, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PN2_ABI_H_ */
