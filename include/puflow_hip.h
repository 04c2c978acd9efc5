/* puflow_hip.h - C ABI of libpuflow_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the native operators under the reference's discrete PU-Flow path.
 * Conventions (shaped like the reference's only native precedent, metric/emd/emd.cpp:14-31):
 *   - every pointer is a DEVICE pointer owned by the caller (contiguous, fp32 / int32);
 *   - the callee allocates nothing, keeps no global state and never synchronises: one call =
 *     stream-ordered enqueue on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - return value: PF_OK (0) or a negative PF_ERR_* code; never throws, never prints;
 *   - scratch comes from the caller (`*_workspace_bytes` queries).
 * No torch types appear here; the Python side (puflow_amd/_lib.py) binds these with ctypes.
 */
#ifndef PUFLOW_HIP_H
#define PUFLOW_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PF_OK 0
#define PF_ERR_NULL (-1)        /* a required pointer is NULL                         */
#define PF_ERR_SHAPE (-2)       /* shape precondition violated                        */
#define PF_ERR_UNSUPPORTED (-3) /* configuration not built (K, unit id, ...)          */
#define PF_ERR_LAUNCH (-4)      /* hipGetLastError() reported a launch failure        */
#define PF_ERR_WORKSPACE (-5)   /* caller workspace too small                         */

int pf_version(void);
const char* pf_error_string(int code);

/* Brute-force kNN. Replaces pytorch3d.ops.knn_points at modules/discrete/interpflow.py:104,:328
 * (and knn_cuda.KNN at modules/utils/patch.py:33,107 for K <= 32).
 * p1 [B,N,3] queries, p2 [B,M,3] references -> idx_out [B,N,K] int32 (index into p2's M),
 * dist_out [B,N,K] squared L2 (nullable).  Order: (distance asc, index asc); distance is the
 * unfused fp32 ((dx*dx)+(dy*dy))+(dz*dz).  K in {4,8,16,32}, K <= M. */
int pf_knn(const float* p1, const float* p2, int B, int N, int M, int K, int* idx_out, float* dist_out, void* stream);

/* Nearest neighbour (K=1): dist_out [B,N] squared L2, idx_out [B,N] (nullable); first minimum
 * wins ties.  Building block of chamfer (pytorch3d.loss.chamfer_distance, metric/loss.py:42;
 * kaolin chamfer, metric/loss.py:35; ChamferDistancePytorch chamfer_3DDist, modules/utils/patch.py:199-203). */
int pf_nn1(const float* p1, const float* p2, int B, int N, int M, float* dist_out, int* idx_out, void* stream);

/* Fused EdgeConv dense block + max-pool over K=16 neighbours, eval mode.
 * Replaces FeatureExtractUnit.forward (modules/discrete/interpflow.py:190-248).
 * cfg 7: units 2..5, cfg 8 / 9: units 0 / 1 - the PRODUCT arithmetic: split-fp16 with a natural-scale low half on
 * v_mfma_f32_16x16x32_f16 (fp32-class results, csrc/pf_mfma.h); wfrag = packing.ec4_weights / ec1n_w (unit 0's edge table
 * rides at the end of its image, input = xyz [B*N,3]); units 1..5 read the P|Q table [B*N, 2S] with the row scales of
 * packing.ec4_scales (csrc/edgeconv.hip edgeconv4_kernel / edgeconv1n_kernel);
 * cfg 0 / 1 / 2: unit 0 (input = xyz, `tab` = [96,8] folded edge table), unit 1, units 2..5 on the exact-fp32 kernel
 * (v_mfma_f32_16x16x4_f32, unscaled P|Q table): the in-library A/B reference the parity tests compare the product with;
 * cfg 3..6 (round-1 split-bf16 / scaled split-fp16 generations) are gone: PF_ERR_UNSUPPORTED.
 * idx [B*N,16] int32 (index inside the batch item); wfrag = fragment-packed growth weights;
 * out [B*N, odim]. */
int pf_edgeconv(int cfg, const float* pq_or_xyz, const float* tab, const int* idx, const float* wfrag, float* out,
                int B, int N, void* stream);

/* Same as pf_edgeconv with an explicit launch shape (points per wave / waves per workgroup).  The default build carries
 * only the shape pf_edgeconv ships per cfg (anything else: PF_ERR_UNSUPPORTED); a -DPF_TUNING_VARIANTS build adds the
 * alternatives and the timing-only ablation instantiations for tools/tune_ec4.py. */
int pf_edgeconv_tuned(int cfg, int variant, const float* pq_or_xyz, const float* tab, const int* idx,
                      const float* wfrag, float* out, int B, int N, void* stream);

/* EdgeConv unit `unit` (0..4, product arithmetic) AND the next unit's P|Q vectors: out [B*N, odim] as pf_edgeconv, pq_next
 * [B*N, rows] as pf_pq_gemm(unit, out, ...) - bit-identical to that pair in every form.  fuse: 0 = the two kernels; 1 = one
 * launch, the GEMM on each 16-point workgroup tile inside the EdgeConv tile loop; 2 = one launch, the GEMM as a tail phase: every
 * workgroup multiplies the tiles it computed itself once its tile loop is done (weights in registers, the LDS weight image as
 * staging area, no synchronisation between workgroups); -1 = by size: form 1 when B*N <= 16 384, above it form 2 for units 0
 * and 2..4 and the two kernels for unit 1; > 2: PF_ERR_UNSUPPORTED.  Forms 1 / 2 fall back to the two kernels when the table is
 * too large for the kernel's 32-bit offsets.  w: weight blob base, off[13]: POST_SLOTS offsets of unit `unit`. */
int pf_edgeconv_pq(int unit, const float* pq_or_xyz, const int* idx, const float* wfrag, float* out, const float* w,
                   const long long* off, float* pq_next, int B, int N, int fuse, void* stream);

/* Per-point stages after EdgeConv unit `unit` (0..5).  off[13] = float offsets into the blob `w` of
 * M1,b1,M2,H1,S2,bS2,T2,bT2,ST4,bST4,PQ,bPQ,scales (packing.POST_SLOTS; f16n fragment images + per-matrix 2^-sw).
 *
 * pf_pq_gemm (unit 0..4): next unit's per-point EdgeConv vectors  PQ' = Wpq h + bpq  -> pq_next [T, 2S']
 *   (the exact per-point fold of the edge feature [x_i, x_j, x_j - x_i], interpflow.py:229-232; packing.fold_edgeconv).
 * pf_cond (unit 0..5): FeatMergeUnit (interpflow.py:251-258), the injector conditioner nets (coupling.py:132-134,
 *   interpflow.py:22-43) and coupling1's c-part: c [T,cdim] (nullable), st [T,8], cp [T,64].
 * pf_post = both, one call per unit (pq_next may be NULL for unit 5 only). */
int pf_pq_gemm(int unit, const float* h, const float* w, const long long* off, float* pq_next, int T, void* stream);
int pf_cond(int unit, const float* h, const float* w, const long long* off, float* c, float* st, float* cp, int T,
            void* stream);
int pf_post(int unit, const float* h, const float* w, const long long* off, float* c, float* st, float* cp,
            float* pq_next, int T, void* stream);
/* Test entry for the layer epilogue of the fused inference kernels (csrc/pf_mfma.h pf_act_pairn): x [n] (n % 8 == 0), every
 * 8 values one pair of 16-channel-block registers.  Writes n / 2 words each of the packed-fp16 hi and lo operand images of
 * the sequence the helper replaces (old_*) and of the helper (new_*); inv == 1 takes the helper's form without rescale. */
int pf_test_act_pairn(const float* x, int n, float inv, float slope, unsigned* old_h, unsigned* old_l, unsigned* new_h,
                      unsigned* new_l, void* stream);
/* pf_cond of all six units in ONE launch (the stages only feed the flow kernels, so they run after the EdgeConv chain):
 * h[6] device pointers to the units' EdgeConv outputs (HOST array of device pointers), c[6] likewise (or NULL),
 * st [6][T][8], cp [6][T][64], off[6*13].  st = cp = NULL with c given: the stage stops at the conditioning features (the
 * continuous model needs nothing else of it). */
int pf_cond_all(const float* const* h, const float* w, const long long* off, float* const* c, float* st, float* cp, int T,
                void* stream);

/* Flow forward f: all 6 FlowBlock.forward in one launch.  Replaces PointInterpFlow.f /
 * FlowBlock.forward (modules/discrete/interpflow.py:302-313,:66-74; normalize.py:30-37,
 * permutate.py:117-120, coupling.py:55-58,114-118,127-139).
 * xyz [T,3]; cp [6][T][64] and st [6][T][8] as written by pf_post (unit-major, contiguous);
 * w = 6 flow records of 5360 floats (layout: csrc/flow.hip header, packing.pack_flow).
 * z [T,3] out; ld_pt [T] out = per-point  -sum_blocks sum_ch s. */
int pf_flow_fwd(const float* xyz, const float* cp, const float* st, const float* w, float* z, float* ld_pt, int T,
                void* stream);

/* Flow inverse g (interpflow.py:315-321,:76-82; coupling.py:82-85,141-151; permutate.py:122-126;
 * normalize.py:39-43): u [T*R,3] (row = n*R + r, conditioning row n) -> x [T*R,3]. */
int pf_flow_inv(const float* u, const float* cp, const float* st, const float* w, float* x, int T, int R, void* stream);

/* Deterministic log-likelihood reduction (PointInterpFlow.log_prob interpflow.py:339-345,
 * probs.py:73-75,87-93):  ldj[b] = sum_n ld_pt + N*ld_const;  lpsum[b] = sum -0.5(z^2+log 2pi) + ldj[b];
 * logp[0] = -mean_b lpsum.  ldj, lpsum: [B] outputs; logp: 1 float. */
int pf_logp(const float* z, const float* ld_pt, float ld_const, int B, int N, float* ldj, float* lpsum, float* logp,
            void* stream);

/* pf_flow_fwd + pf_logp in ONE launch (the workgroup that finishes last reduces the wave tiles' sums per batch item, in a
 * fixed order): outputs as those two.  ws: pf_flow_fwd_logp_ws_floats(B, N) floats, ZERO before the first call and left
 * reusable by the kernel; one workspace per stream in flight.  N % 16 != 0 runs the two launches. */
long long pf_flow_fwd_logp_ws_floats(int B, int N);
int pf_flow_fwd_logp(const float* xyz, const float* cp, const float* st, const float* w, float* z, float* ld_pt,
                     float ld_const, int B, int N, float* ldj, float* lpsum, float* logp, float* ws, void* stream);

/* Interpolation module (interpflow.py:85-186), fused: kNN-8 context features -> weights ->
 * softmax_k -> weighted sum of neighbour latents.  idx16 [T,16] (first 8 columns used),
 * u_out [T*R,3] in the row order of g (row = n*R + r).  1 <= R <= 32 (r_max of WeightEstimationUnit,
 * interpflow.py:142; R <= 4 runs the 4-row fast path, larger ratios all 32 rows of the last weight conv).
 * off[15]: float offsets into w (csrc/interp.hip header, packing.INTERP_SLOTS); the blob does not depend on R. */
int pf_interp(const float* xyz, const float* z, const int* idx16, const float* w, const long long* off, float* u_out,
              int B, int N, int R, void* stream);

/* The same module split so that its heavy part does not wait for the latents: pf_interp_weights writes the softmax weights
 * aw [B*N][8][4] (a function of xyz and the neighbour lists only: it can run beside the feature extractor / flow f chain, e.g.
 * as a parallel branch of a captured graph), pf_flow_inv_interp forms u[n R + r] = sum_k aw[n][k][r] z[idx8[n][k]] inside the
 * flow-g kernel.  R <= 4.  The pair returns the bits of pf_interp followed by pf_flow_inv. */
int pf_interp_weights(const float* xyz, const int* idx16, const float* w, const long long* off, float* aw_out, int B, int N,
                      void* stream);
int pf_flow_inv_interp(const float* aw, const float* z, const int* idx16, const float* cp, const float* st, const float* w,
                       float* x, int B, int N, int R, void* stream);

/* Chamfer forward: dist1/idx1 [B,N] (x -> y), dist2/idx2 [B,M] (y -> x), squared L2, first-minimum ties.
 * per_sample [B] = mean_n dist1 + mean_m dist2 (nullable); mean_sum [2] = {mean_b, sum_b} of per_sample
 * (nullable).  Replaces pytorch3d chamfer_distance (metric/loss.py:42), kaolin chamfer (metric/loss.py:35)
 * and chamfer_3DDist (modules/utils/patch.py:199-203). */
int pf_chamfer_fwd(const float* x, const float* y, int B, int N, int M, float* dist1, int* idx1, float* dist2,
                   int* idx2, float* per_sample, float* mean_sum, void* stream);

/* Chamfer backward: g1 [B,N] = dL/d dist1, g2 [B,M] = dL/d dist2; ACCUMULATES into gx [B,N,3], gy [B,M,3]
 * (caller zero-fills).  d dist/d x_i = 2 (x_i - y_j), d dist/d y_j = -2 (x_i - y_j). */
int pf_chamfer_bwd(const float* x, const float* y, const int* idx1, const int* idx2, const float* g1, const float* g2,
                   float* gx, float* gy, int B, int N, int M, void* stream);
/* the same without float atomics (every point's incoming terms found by a scan of the other cloud's nearest-neighbour map and
 * added in index order): bit-reproducible, O(N M) per sample - the training step's debugging switch (PF_TRAIN_DETERMINISTIC) */
int pf_chamfer_bwd_det(const float* x, const float* y, const int* idx1, const int* idx2, const float* g1, const float* g2,
                       float* gx, float* gy, int B, int N, int M, void* stream);

/* Auction EMD forward.  Replaces emd.forward (metric/emd/emd.cpp:14-19 -> emd_cuda.cu:228-282).
 * Same ownership rule as the reference: the caller allocates outputs AND scratch (emd_module.py:43-56):
 * xyz1 (prediction), xyz2 (ground truth) [B,n,3]; dist [B,n] out; assignment [B,n] in/out (-1 = free);
 * price [B,n] in/out (0); assignment_inv [B,n] in/out (-1); bid, bid_increments, max_increments,
 * unass_idx, max_idx: [B,n] scratch.  The reference's unass_cnt / unass_cnt_sum / cnt_tmp (512-entry
 * batch prefix sums for its multi-kernel pipeline) have no counterpart: one workgroup owns one sample.
 * No n % 1024 or B <= 512 restriction.  Returns PF_OK / PF_ERR_* (the reference returns 1 / 0 / -1). */
int pf_emd_forward(const float* xyz1, const float* xyz2, float* dist, int* assignment, float* price,
                   int* assignment_inv, int* bid, float* bid_increments, float* max_increments, int* unass_idx,
                   int* max_idx, float eps, int iters, int B, int n, void* stream);

/* pf_emd_forward with the launch decision and the failure report made explicit.
 * groups: workgroups per sample.  0 = chosen here from the device: the multi-workgroup auction waits on grid barriers, so it
 * runs only when hipOccupancyMaxActiveBlocksPerMultiprocessor(kernel) x CU count says all B*G workgroups are resident at once
 * (G = largest power of two <= 16 that fits, >= 64 points per workgroup), otherwise one workgroup per sample; 1 = always one
 * workgroup per sample (no inter-workgroup waits: the setting for a GPU shared between processes); g > 1 = at most g.
 * status: nullable device word; += 1 per WORKGROUP whose barrier timed out (its slice of dist is NaN): any non-zero value is
 * a failure.  The caller reads it
 * at its next synchronisation point (puflow_amd.loss.check_emd_status raises). */
int pf_emd_forward_ex(const float* xyz1, const float* xyz2, float* dist, int* assignment, float* price,
                      int* assignment_inv, int* bid, float* bid_increments, float* max_increments, int* unass_idx,
                      int* max_idx, float eps, int iters, int B, int n, int groups, unsigned* status, void* stream);

/* Auction EMD backward.  Replaces emd.backward (emd.cpp:21-24 -> emd_cuda.cu:284-316):
 * gradxyz [B,n,3] += 2 graddist (xyz1 - xyz2[idx]); gradient wrt xyz2 is zero (emd_module.py:68-72). */
int pf_emd_backward(const float* xyz1, const float* xyz2, float* gradxyz, const float* graddist, const int* idx, int B,
                    int n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training-step building blocks (csrc/train_gemm.hip: the matrix products, csrc/train_ops.hip: the rest): one kernel pair
 * per eager op the reference's train-mode forward/backward runs (modules/discrete/interpflow.py:203-258,
 * train_pu1k.py:53-74), on channels-last [rows, C] fp32 tensors.  Wired into autograd by puflow_amd/train_perop.py.
 * ------------------------------------------------------------------------------------------- */

/* C[M,N] = A(M,K) B(K,N) (+ bias[N]), generic element strides: A(m,k) = A[m*sam + k*sak], B(k,n) = B[k*sbk + n*sbn].
 * Serves every Conv2d(1x1) / nn.Linear forward, dX and dW.  ws: split-K slabs, pf_gemm_ws_floats(M,N,K) floats. */
long long pf_gemm_ws_floats(int M, int N, int K);
int pf_gemm(const float* A, long long sam, long long sak, const float* B, long long sbk, long long sbn, float* C,
            long long ldc, const float* bias, int M, int N, int K, float* ws, long long ws_floats, void* stream);
/* the split-K reduction of pf_gemm for callers that wrote their own slabs [nslab][M * N]: C [M, ldc] = their sum, fixed order */
int pf_gemm_reduce(const float* slabs, float* C, int M, int N, long long ldc, int nslab, void* stream);
/* pf_gemm with the matrix-pipe arithmetic chosen by the caller: 0 = f32 MFMA (what pf_gemm runs: the float4-load kernel where
 * the operands allow it, else the general one), 1 = the same products in the same order on the general kernel (any strides,
 * scalar loads) whatever the operands (reference: bit-identical to 0), 2 = split-fp16 (operands
 * inside the fp16 range: forward GEMMs), 3 = split-bf16 (gradient operands); all fp32-class results. */
int pf_gemm_ex(int arith, const float* A, long long sam, long long sak, const float* B, long long sbk, long long sbn, float* C,
               long long ldc, const float* bias, int M, int N, int K, float* ws, long long ws_floats, void* stream);

/* BatchNorm2d(training) + LeakyReLU(slope) on x [R,C] (interpflow.py:205-206,216-217; eps 1e-5, momentum 0.1):
 * save [2][C] = batch mean, 1/sqrt(var+eps); running stats updated in place when non-NULL (unbiased variance).
 * ws: (2*pf_bn_chunks(R) + 2) * C floats. */
int pf_bn_chunks(long long R);
int pf_bn_lrelu_fwd(const float* x, long long R, int C, const float* gamma, const float* beta, float slope, float eps,
                    float momentum, float* run_mean, float* run_var, float* y, float* save, float* ws, void* stream);
int pf_bn_lrelu_bwd(const float* x, const float* dy, long long R, int C, const float* gamma, const float* beta, float slope,
                    const float* save, float* dx, float* dgamma, float* dbeta, float* ws, void* stream);
/* The same BatchNorm + LeakyReLU in stages, so that per-column sums can be all-reduced between them (SyncBN across
 * ranks; SURVEY 8e "decision to document" / f-3).  Sums are unscaled; the host divides by the global row count.
 *   pf_bn_colstat:     out[c] = sum_r x (mean_in NULL) or sum_r (x - mean_in)^2;   ws: 2*pf_bn_chunks(R)*C floats
 *   pf_bn_apply_stats: y from GIVEN mean / biased variance; save = [mean | invstd]; running stats updated (nullable)
 *   pf_bn_bwd_sums:    sums[2][C] = (sum dz, sum dz*xhat) of this rank's rows (= dbeta, dgamma of the local loss)
 *   pf_bn_bwd_apply:   dx from the global means[2][C] = all-reduced sums / global row count */
int pf_bn_colstat(const float* x, long long R, int C, const float* mean_in, float* out, float* ws, void* stream);
int pf_bn_apply_stats(const float* x, long long R, int C, const float* mean, const float* var_b, float unbias,
                      const float* gamma, const float* beta, float slope, float eps, float momentum, float* run_mean,
                      float* run_var, float* y, float* save, void* stream);
int pf_bn_bwd_sums(const float* x, const float* dy, long long R, int C, const float* gamma, const float* beta, float slope,
                   const float* save, float* sums, float* ws, void* stream);
int pf_bn_bwd_apply(const float* x, const float* dy, long long R, int C, const float* gamma, const float* beta, float slope,
                    const float* save, const float* means, float* dx, void* stream);
/* column sums of g [R,C] -> out [C] (bias gradients); ws: 2*pf_bn_chunks(R)*C floats */
int pf_colsum(const float* g, long long R, int C, float* out, float* ws, void* stream);

/* y = x > 0 ? x : slope*x (LeakyReLU; slope 0 = ReLU) and its backward from the OUTPUT sign */
int pf_act_fwd(const float* x, float slope, long long total, float* y, void* stream);
int pf_act_bwd(const float* y, const float* dy, float slope, long long total, float* dx, void* stream);

/* EdgeConv edge feature (interpflow.py:223-232): out [B*N*K, 3C] = [x_i, x_j, x_j - x_i]; backward ACCUMULATES into dx */
int pf_edge_feature_fwd(const float* x, const int* idx, int B, int N, int K, int C, float* out, void* stream);
int pf_edge_feature_bwd(const float* g, const int* idx, int B, int N, int K, int C, float* dx, void* stream);

/* max over the K neighbours (interpflow.py:245): y [T,K,C] -> out [T,C], arg [T,C]; backward dx [T,K,C] */
int pf_maxpool_k_fwd(const float* y, long long T, int K, int C, float* out, int* arg, void* stream);
int pf_maxpool_k_bwd(const float* dy, const int* arg, long long T, int K, int C, float* dx, void* stream);

/* backward of a neighbour-row gather x[idx] (interpflow.py:183): out [B*N,C] += g [B*N*K,C] (out zero-filled by caller) */
int pf_scatter_rows(const float* g, const int* idx, int B, int N, int K, int C, float* out, void* stream);
/* the same as a gather over the sorted transposed lists of idx (pf_knn_csr): out [T, C] = sum over the edges that point at a row,
 * in list order - no float atomics (PF_TRAIN_DETERMINISTIC) */
int pf_scatter_rows_det(const float* g, const int* csr_off, const int* csr_edge, long long T, int C, float* out, void* stream);
/* backward of repeat_interleave(c, R, dim=1) (interpflow.py:319): out [T,C] = sum_r g[T*R,C] */
int pf_group_sum(const float* g, long long T, int R, int C, float* out, void* stream);

/* interpolation tail (interpflow.py:180-185): softmax over K=8 of the first R channels of w [T,K,ldw], weighted sum of
 * the gathered latents zj [T,K,3] -> a [T,K,R], fz [T,3,R]; backward -> dw [T,K,ldw], dzj [T,K,3] */
int pf_softmax_wsum_fwd(const float* w, int ldw, const float* zj, int K, int R, long long T, float* a, float* fz,
                        void* stream);
int pf_softmax_wsum_bwd(const float* a, const float* zj, const float* dfz, int K, int R, int ldw, long long T, float* dw,
                        float* dzj, void* stream);

/* Flow-block elementwise algebra on [R,3] rows for the training path (csrc/train_ops.hip, second part), forward +
 * backward: ActNorm (normalize.py:30-43; inv = 1: (x-bias) exp(-logs)); additive coupling + channel reverse + injector
 * (coupling.py:55-58,114-118,132-137; permutate.py:75-80) and their inverse halves (coupling.py:82-85,141-151);
 * per-batch sums for the log-det and the Gaussian log-likelihood (probs.py:73-75,87-93).  td = width of the first
 * split (1 or 2).  Parameter-gradient rows (glogs_rows, gbias_rows [R,3]) are column-summed with pf_colsum. */
int pf_actnorm_fwd(const float* x, const float* logs, const float* bias, int inv, long long R, float* y, void* stream);
int pf_actnorm_bwd(const float* x, const float* dy, const float* logs, const float* bias, int inv, long long R, float* dx,
                   float* glogs_rows, float* gbias_rows, void* stream);
int pf_couple_inject_fwd(const float* y, const float* o, const float* s, const float* t, int td, long long R, float* out,
                         void* stream);
int pf_couple_inject_bwd(const float* out, const float* dout, const float* s, int td, long long R, float* dy, float* do_,
                         float* ds, float* dt, void* stream);
int pf_inject_inv_fwd(const float* u, const float* s, const float* t, long long R, float* v, void* stream);
int pf_inject_inv_bwd(const float* u, const float* s, const float* dv, long long R, float* du, float* ds, float* dt,
                      void* stream);
int pf_couple_add(const float* v, const float* o, int td, long long R, float* out, void* stream);
int pf_slice_tail(const float* g, int td, long long R, float* o, void* stream);
/* out[b] = sum_m f(x[b*M+m]); mode 0: f = x, mode 1: f = -0.5 (x^2 + log 2 pi); backward dx = g[b] f'(x) */
int pf_batch_sum_fwd(const float* x, int B, long long M, int mode, float* out, void* stream);
int pf_batch_sum_bwd(const float* x, const float* g, int B, long long M, int mode, float* dx, void* stream);
/* DistanceEncoder.distance_vec (interpflow.py:100-115): out [B*N*K,10] = [x_i, x_j, x_i - x_j, |x_i - x_j|] */
int pf_dist_feature(const float* xyz, const int* idx, int B, int N, int K, float* out, void* stream);

/* ---- one FeatureExtractUnit (EdgeConv dense block) of the training step, fused (csrc/pf_ec_train.h: train_ec_fwd.hip, train_fused.hip) ----
 * Replaces FeatureExtractUnit.forward in train() mode and its autograd backward (modules/discrete/interpflow.py:190-248):
 * edge feature -> [Conv2d 1x1 + BatchNorm2d(batch statistics) + LeakyReLU, dense concatenation] x nconv -> conv_out ->
 * max over the K neighbours (pooling = 1) or the per-edge output (pooling = 0, the interpolation's feat_conv).
 * T = B*N points, E = T*K edges (point-major rows), GT = growth*nconv, S = GT + odim.  growth in {8,16,32}, nconv <= 8,
 * odim a multiple of 16 <= 128, GT in {32, 64, 128}, E a multiple of 16, pooling requires K == 16.
 * The caller owns every buffer; those marked (kept) must survive from pf_ec_train_fwd to pf_ec_train_bwd. */
#define PF_TRAIN_STAT_DOUBLES 4097
typedef struct PfEcTrain {
    int B, N, K, C, growth, nconv, odim, pooling;
    float slope, eps, momentum;
    const float* x;                 /* [T, C] */
    const int* idx;                 /* [T, K] batch-local neighbour indices */
    const float* W[9];              /* conv t [growth, 3C + growth t] (t < nconv), then conv_out [odim, 3C + GT] */
    const float* bias[9];
    const float* gamma[8]; const float* beta[8];
    float* run_mean[8]; float* run_var[8];     /* nullable: running statistics, updated in place */
    float* Wpq;                     /* (kept) [2S, C] folded edge-feature weights */
    float* bpq;                     /* [2S] */
    float* PQ;                      /* (kept) [T, 2S] */
    float* Y;                       /* (kept) [E, GT] pre-BatchNorm outputs of the growth layers */
    float* aff;                     /* (kept) [4][GT] scale, shift, batch mean, 1/std */
    float* out;                     /* [T, odim] (pooling) or [E, odim] */
    unsigned char* arg;             /* (kept) [T, odim] argmax over K (pooling) */
    /* backward only */
    const float* dout;              /* gradient of `out` */
    float* dA;                      /* [E, GT] scratch */
    float* dPQ;                     /* [T, 2S] scratch */
    float* coef;                    /* [2][GT] scratch */
    float* dWpq;                    /* [2S, C] scratch */
    float* dx;                      /* [T, C], nullable */
    float* dW[9]; float* dbias[9]; float* dgamma[8]; float* dbeta[8];
    float* ws; long long ws_floats; /* >= pf_ec_train_ws_floats() */
    double* stat;                   /* PF_TRAIN_STAT_DOUBLES doubles (column-statistics accumulators): zeroed ONCE by the caller,
                                       every kernel that uses them leaves them zero again */
    const int* csr_off; const int* csr_edge;   /* backward, nullable: transposed neighbour lists (pf_knn_csr) - the neighbour
                                       scatter-add of dQ then runs as a gather without float atomics */
    int flags;                      /* PF_EC_PERSISTENT: the forward may run as ONE persistent launch with a grid barrier per
                                       BatchNorm layer (pooling units, K = 16, nconv = 4, every tile resident at once - decided by
                                       the library from the device's occupancy).  The caller sets it only when no other barrier
                                       kernel of the process can run beside this call (another stream, another captured graph in
                                       flight, another process on the device): two such kernels can starve each other */
    unsigned* sync;                 /* flags != 0: 4 words, zeroed ONCE by the caller; [0..2] are left zero by every launch, [3] is
                                       sticky: 1 = a grid barrier timed out (the unit's output is NaN) */
    /* SyncBN (BatchNorm statistics over all ranks, interpflow.py:93,96,205,216 with global-batch semantics): sync_sums != NULL
     * makes every BatchNorm layer leave its LOCAL column sums + row count in sync_sums (2 * 128 + 1 doubles) instead of
     * finishing; the library then calls sync_cb(sync_user, sync_sums, 257, stream) - which must all-reduce (SUM) those doubles
     * over the ranks, stream-ordered, and return 0 - and finishes the layer with the global sums in one small launch.  dgamma /
     * dbeta stay the local sums (as torch.nn.SyncBatchNorm: the gradient bucket's mean over ranks follows).  The persistent
     * launches are not used in this mode. */
    int (*sync_cb)(void* user, double* sums, int n, void* stream);
    void* sync_user;
    double* sync_sums;
    float* ws_dw; long long ws_dw_floats; /* backward with pf_train_set_dw_stream: a second workspace (>= pf_ec_train_ws_floats()) that
                                     * only the weight-gradient stream's kernels use; NULL = weight gradients on the calling stream */
    const float* dx_add;            /* backward, nullable: [B*N, C] added to dx in the epilogue of its GEMM - the part of x's gradient
                                     * that x's OTHER consumer (the unit's FeatMergeUnit, interpflow.py:251-258) has produced already,
                                     * instead of a separate add launch afterwards */
} PfEcTrain;
#define PF_EC_PERSISTENT 1
/* flags bit (PfEcTrain, PfBnMlpTrain): BatchNorm's batch statistics are accumulated as 64-bit fixed-point sums with integer
 * atomics instead of double atomics - exact, hence independent of the order in which workgroups arrive: two runs of the same
 * step give the same bits (the default's double sums round in arrival order once they need more than 53 bits, and a 1e-7
 * difference in x flips discrete auction assignments and max-pool routes).  Each workgroup partial is split into two words,
 * quanta 2^-28 (range |sum| < 3.4e10) and 2^-60, in the same PF_TRAIN_STAT_DOUBLES accumulators: ~4e-19 absolute per partial.
 * Measured against float64 with BatchNorm gradients scaled down to 1e-5 (a batch-mean loss's): at most 8.5e-5 of the largest,
 * the default mode's figure on the same inputs (a single 2^-28 word missed them by 3.3e-3 to 1.0e-2).  The persistent kernels are not used under it.  Debugging switch:
 * puflow_amd sets it from `net.deterministic` / `cfg.deterministic`. */
#define PF_TRAIN_DETERMINISTIC 2
/* flags bit (PfEcTrain): Wpq / bpq were filled by pf_ec_train_fold_batch since the parameters last changed - pf_ec_train_fwd
 * skips its own fold launch */
#define PF_EC_PREFOLDED 4
/* transposed neighbour lists of idx [B*N, K]: off [T+1], edge [T*K]; cnt: T ints (4-aligned size) of scratch */
/* Weight gradients beside the backward chain.  With a stream set here (per host thread; NULL = off, the default) the backward
 * entry points pf_ec_train_bwd, pf_mlp_train_bwd, pf_mlp_train_bwd_batch and pf_mlp_train_dw_batch enqueue their split-K
 * weight-gradient kernels and reductions on it, ordered by an event behind what their own stream holds at that point, and
 * return without waiting: the input gradient stays on the calling stream.  The caller (1) hands those calls workspaces that
 * nothing on another stream touches (PfEcTrain.ws_dw; PfMlpTrain.ws is weight-gradient scratch only), (2) keeps every buffer
 * of the call alive until (3) it has made the consumer of the weight gradients wait for the stream.  Inside a hipGraph
 * capture the stream must belong to the capture (it joins it through the event) and is a parallel branch of the graph. */
int pf_train_set_dw_stream(void* stream);
int pf_knn_csr(const int* idx, int B, int N, int K, int* off, int* edge, int* cnt, void* stream);
/* pf_knn_csr for idx [B*N, K] and for its first K2 <= K columns (as if those were stored contiguously: edge ids i K2 + k) from one
 * pass: off [T+1], edge [T*K], off2 [T+1], edge2 [T*K2]; cnt: 2 x ((T + 3) / 4 * 4) ints of scratch.  The training step uses both
 * (16 neighbours: feature units, 8: the interpolation unit, interpflow.py:85-151,300-306). */
int pf_knn_csr_pair(const int* idx, int B, int N, int K, int K2, int* off, int* edge, int* off2, int* edge2, int* cnt, void* stream);

/* sorts every list of pf_knn_csr (edge ids ascending; T = B*N lists): sums over a list then add in one order, run after run -
 * what PF_TRAIN_DETERMINISTIC's gather-form gradients need; the default mode does not call it */
int pf_knn_csr_sort(const int* off, int* edge, int T, void* stream);
long long pf_ec_train_ws_floats(const PfEcTrain* p);
int pf_ec_train_fwd(const PfEcTrain* p, void* stream);
/* The folded edge-feature weights Wpq / bpq of n <= 8 units (only C, growth, nconv, odim, B, N, K, W, bias, Wpq, bpq of each
 * descriptor are read) in ONE launch: they depend on parameters only (interpflow.py:190-248 applies the convolutions to
 * cat[x_i, x_j, x_j - x_i]; W_p = W_a - W_c, W_q = W_b + W_c), so a step folds all units before the first one runs. */
int pf_ec_train_fold_batch(const PfEcTrain* descs, int n, void* stream);
int pf_ec_train_bwd(const PfEcTrain* p, void* stream);

/* ---- BatchNorm MLP of the interpolation module in the training step, fused (csrc/train_bnmlp.hip) ----
 * Replaces DistanceEncoder.mlp / WeightEstimationUnit.mlp (modules/discrete/interpflow.py:85-151: [Conv2d 1x1 +
 * BatchNorm2d(batch statistics) + LeakyReLU(slope)] x (nl - 1), then Conv2d 1x1) in train() mode with their autograd
 * backward.  Input = cat[xa [rows, kin0a], xb [rows, kin0b]] (never built; kin0b = 0: one input); widths multiples of 16
 * <= 128, kin0a, kin0b <= 128.  W[l]: [width[l], in_l], in_0 = kin0a + kin0b. */
typedef struct PfBnMlpTrain {
    int rows, nl, kin0a, kin0b;
    int width[3];
    float slope, eps, momentum;
    const float* xa; const float* xb;
    const float* W[3]; const float* b[3];
    const float* gamma[2]; const float* beta[2];
    float* run_mean[2]; float* run_var[2];      /* nullable */
    float* y[3];                    /* (kept) [rows, width[l]] pre-BatchNorm output of layer l; y[nl-1] is the result */
    float* aff[2];                  /* (kept) [4][width[l]] scale, shift, batch mean, 1/std */
    /* backward only */
    const float* dout;              /* [rows, width[nl-1]] */
    float* d[2];                    /* [rows, width[l]] scratch */
    float* coef[2];                 /* [2][width[l]] scratch */
    float* dxa; float* dxb;         /* nullable: [rows, kin0a], [rows, kin0b] */
    float* dW[3]; float* db[3]; float* dgamma[2]; float* dbeta[2];
    float* ws; long long ws_floats; /* >= pf_bnmlp_train_ws_floats() */
    double* stat;                   /* PF_TRAIN_STAT_DOUBLES doubles, zeroed once by the caller (see PfEcTrain) */
    int (*sync_cb)(void* user, double* sums, int n, void* stream);      /* SyncBN, as in PfEcTrain */
    void* sync_user;
    double* sync_sums;
    int flags;                      /* PF_TRAIN_DETERMINISTIC, PF_BNMLP_SUM_INPUTS */
} PfBnMlpTrain;
/* PfBnMlpTrain.flags: layer 0 is no product - its pre-BatchNorm output is xa + xb (kin0a = kin0b = width[0]; W[0], b[0], dW[0],
 * db[0], dxa, dxb unused: the gradient of BOTH inputs is d[0] after the backward call).  For a first layer whose weights were
 * folded into the last linear layers of the two producers (WeightEstimationUnit's conv 0 over cat[DistanceEncoder, EdgeConv],
 * modules/discrete/interpflow.py:134,144-146: no nonlinearity between them) - the same function, 2 x 128 x 128 MACs per row less. */
#define PF_BNMLP_SUM_INPUTS 4
long long pf_bnmlp_train_ws_floats(const PfBnMlpTrain* p);
int pf_bnmlp_train_fwd(const PfBnMlpTrain* p, void* stream);
int pf_bnmlp_train_bwd(const PfBnMlpTrain* p, void* stream);

/* ---- point-wise MLP of the training step (2 or 3 Linear layers, LeakyReLU / ReLU between them), fused (csrc/train_mlp.hip) ----
 * Replaces LinearA1D (modules/discrete/interpflow.py:22-43, the conditioner of the coupling / injector layers) and
 * FeatMergeUnit (interpflow.py:251-258) in train() mode together with their autograd backward.
 * Input of layer 0 = cat[y[row, :td], c[row / cdiv, :cc]] (never materialised): td <= 3, cc a multiple of 16 <= 128,
 * cdiv in {1,2,4,8,16} divides rows; hidden widths multiples of 16 <= 128; last width <= 128.
 * W[l]: [width[l], in_l] row-major, in_0 = td + cc, in_l = width[l-1]; b[l] nullable. */
typedef struct PfMlpTrain {
    int rows, nl, td, ldy, cc, cdiv;
    int width[3];
    float slope[2];                 /* activation after layer 0 (and 1): max(x, slope x) */
    const float* y;                 /* [rows, ldy], nullable when td == 0 */
    const float* c;                 /* [rows / cdiv, cc] */
    const float* W[3]; const float* b[3];
    float* h[2];                    /* (kept) [rows, width[l]] activations after layer l < nl - 1 */
    float* out;                     /* [rows, width[nl-1]] */
    /* backward only */
    const float* dout;
    float* dz[2];                   /* [rows, width[l]] scratch */
    float* dy;                      /* [rows, ldy] (columns >= td zeroed), nullable */
    float* dc;                      /* [rows / cdiv, cc], nullable */
    float* dW[3]; float* db[3];     /* db[l] nullable */
    float* ws; long long ws_floats; /* >= pf_mlp_train_ws_floats() */
    int chunk;                      /* rows per split-K chunk of the weight-gradient launch: 0 = default, else a multiple of 32 */
    int flags;                      /* PF_MLP_DW_DZSUM (pf_mlp_train_dw_batch only; 0 everywhere else) */
} PfMlpTrain;
/* PfMlpTrain.flags, pf_mlp_train_dw_batch with cdiv > 1 and cc a multiple of 16: `dc` is an INPUT - [rows / cdiv, width[0]], the sum
 * of dz[0] over the cdiv consecutive rows that share a conditioning row (pf_flowchain_bwd writes it: PfFlowChain.dz1s).  The
 * conditioning columns of layer 0's weight gradient are then accumulated over the rows / cdiv summed rows,
 *   sum_rows dz0[row]^T c[row / cdiv] = sum_points (sum_r dz0[point cdiv + r])^T c[point],
 * and only the td <= 3 coordinate columns over all rows: a third of the layer's matrix work at cdiv = 4, same value up to the
 * order of the additions. */
#define PF_MLP_DW_DZSUM 1
long long pf_mlp_train_ws_floats(const PfMlpTrain* p);
int pf_mlp_train_fwd(const PfMlpTrain* p, void* stream);
int pf_mlp_train_bwd(const PfMlpTrain* p, void* stream);
/* n <= 16 networks of the same depth in one launch per kernel (blockIdx.z = network), e.g. the scale / shift conditioners of
 * all flow blocks, which depend only on the conditioning features.  dev_descs: n * sizeof(PfMlpTrain) bytes of device
 * scratch. */
int pf_mlp_train_fwd_batch(const PfMlpTrain* descs, int n, void* dev_descs, void* stream);
int pf_mlp_train_bwd_batch(const PfMlpTrain* descs, int n, void* dev_descs, void* stream);

/* Weight gradients only (split-K launch + reduction) of n <= 16 networks whose dz / h / dout are already in memory
 * (written by pf_flowchain_bwd); same descriptors as pf_mlp_train_bwd_batch. */
int pf_mlp_train_dw_batch(const PfMlpTrain* descs, int n, void* dev_descs, void* stream);

/* ---- all flow blocks of one direction of the training step: two launches forward, four backward (csrc/train_flowchain.hip) ----
 * Replaces PointInterpFlow.f / .g over FlowBlock.forward / .inverse (modules/discrete/interpflow.py:46-82, 302-321) in train()
 * mode: ActNorm (normalize.py:28-54), the invertible 3x3 linear (permutate.py:117-124), the additive coupling with its LinearA1D
 * conditioner on cat[coords[:td], c] (coupling.py:55-58,114-118; interpflow.py:22-43; hidden width 64, 32 / 64 / 128
 * conditioning channels), the reverse permutation (permutate.py:77-80) and the conditional affine injector with s, t given per ORIGINAL
 * point (coupling.py:120-137).  inv = 0: x [T,3] -> z, ssum[i] = sum(s_i), ld[i] = (sum(logs_i) + log|det W_i|) n_ld;
 * inv = 1: u [T R, 3] -> x through the blocks in reverse order, conditioning rows shared by R in {1,2,4,8,16} consecutive rows.
 * Slabs (`pin`, `mid`, `o`, `h1`, `h2`, `dz1`, `dz2`, `dob`) are indexed by block and kept between forward and backward.
 * Backward: dout [rows,3] (+ dssum, dld [nb], nullable) -> dx (nullable), dc[i] [rows / R, cc[i]], ds[i], dt[i] [rows / R, 3] and
 * every parameter gradient.  part: pf_flowchain_part_floats() floats (both directions); counter: one zero word (left zero); ws:
 * pf_flowchain_ws_floats() floats; dev_descs: nb * sizeof(PfMlpTrain) bytes. */
#define PF_FLOWCHAIN_MAXB 8
typedef struct PfFlowChain {
    int nb, rows, R, inv;
    int td[PF_FLOWCHAIN_MAXB];       /* untouched leading coordinates of block i's coupling (1 or 2) */
    int cc[PF_FLOWCHAIN_MAXB];       /* conditioning channels of block i (32, 64 or 128) */
    float n_ld;                      /* inv = 0: points per batch item (factor of the log-determinant) */
    const float* x;                  /* [rows, 3] */
    const float* c[PF_FLOWCHAIN_MAXB];                                       /* [rows / R, cc[i]] */
    const float* s[PF_FLOWCHAIN_MAXB]; const float* t[PF_FLOWCHAIN_MAXB];    /* [rows / R, 3] */
    const float* logs[PF_FLOWCHAIN_MAXB]; const float* bias[PF_FLOWCHAIN_MAXB]; const float* W[PF_FLOWCHAIN_MAXB];
    const float* w0[PF_FLOWCHAIN_MAXB];                                      /* [64, td + cc] (no bias) */
    const float* w2[PF_FLOWCHAIN_MAXB]; const float* b2[PF_FLOWCHAIN_MAXB];  /* [64, 64], [64] */
    const float* w4[PF_FLOWCHAIN_MAXB]; const float* b4[PF_FLOWCHAIN_MAXB];  /* [3 - td, 64], [3 - td] */
    float* pin; float* mid;          /* [nb][rows, 3]: block input; y (inv = 0) / v (inv = 1) */
    float* o;                        /* [nb][rows, 2] coupling shift (inv = 1) */
    float* h1; float* h2;            /* [nb][rows, 64] */
    float* out;                      /* [rows, 3] */
    float* ssum; float* ld;          /* [nb] (inv = 0) */
    float* logp; int Bsz;            /* inv = 0, nullable: logp[0] = -(sum_rows log N(z) / Bsz + sum_i ld_i - sum_i ssum_i / Bsz), nb <= 7 */
    float* part; unsigned* counter;
    float* img;                      /* pf_flowchain_img_floats(): packed weights, written by the forward, read by the backward */
    /* backward only */
    const float* dout; const float* dssum; const float* dld;
    const float* dlogp;              /* gradient of logp[0]; replaces dssum / dld when given (dout then nullable) */
    float* dx;
    float* dc[PF_FLOWCHAIN_MAXB]; float* ds[PF_FLOWCHAIN_MAXB]; float* dt[PF_FLOWCHAIN_MAXB];
    float* dz1; float* dz2;          /* [nb][rows, 64] */
    float* dob;                      /* [nb] slabs of rows * 2 floats; slab i holds [rows, 3 - td_i] */
    float* dlogs[PF_FLOWCHAIN_MAXB]; float* dbias[PF_FLOWCHAIN_MAXB]; float* dW[PF_FLOWCHAIN_MAXB];
    float* dw0[PF_FLOWCHAIN_MAXB]; float* dw2[PF_FLOWCHAIN_MAXB]; float* db2[PF_FLOWCHAIN_MAXB];
    float* dw4[PF_FLOWCHAIN_MAXB]; float* db4[PF_FLOWCHAIN_MAXB];
    float* ws; long long ws_floats;
    void* dev_descs;
    float* dz1s;                     /* backward, nullable, R > 1: [nb][rows / R, 64] = dz1 summed over the R rows of a conditioning
                                      * row - with it the weight-gradient launch runs layer 0's conditioning columns over rows / R
                                      * summed rows (PF_MLP_DW_DZSUM) */
    int img_ready;                   /* forward: img already holds the packed weights of these parameters (the other direction's call
                                      * of the same forward packed them: the image does not depend on inv / R) - no pack launch */
} PfFlowChain;
long long pf_flowchain_ws_floats(const PfFlowChain* a);
long long pf_flowchain_part_floats(const PfFlowChain* a);
long long pf_flowchain_img_floats(const PfFlowChain* a);
int pf_flowchain_fwd(const PfFlowChain* a, void* stream);
int pf_flowchain_bwd(const PfFlowChain* a, void* stream);

/* ---- element-wise half of a flow block in the training step, fused per direction (csrc/train_flow.hip) ----
 * Replaces ActNorm / InvertibleConv1x1-style 3x3 linear / AffineCoupling / reverse permutation / AffineInjector of
 * modules/discrete/interpflow.py:46-82 (normalize.py:28-54, permutate.py:77-124, coupling.py:55-137) in train() mode.
 * partial: >= 256 * 15 floats of scratch; counter: one 32-bit word, zero between calls. */
int pf_flow_params_fwd(const float* W, const float* logs, float n, float* Winv, float* ld, void* stream);
int pf_flow_params_bwd(const float* Winv, const float* dWinv, const float* dld, float n, float* dW, float* dlogs, void* stream);
int pf_flow_affine_fwd(const float* x, const float* o, int td, const float* logs, const float* bias, const float* M, int inv,
                       long long R, float* y, void* stream);
int pf_flow_affine_bwd(const float* x, const float* o, int td, const float* logs, const float* bias, const float* M, int inv,
                       long long R, const float* dy, float* dx, float* dobuf, float* dlogs, float* dbias, float* dM,
                       float* partial, unsigned* counter, void* stream);
int pf_couple_inject2_fwd(const float* y, const float* o, const float* s, const float* t, int td, long long R, float* out,
                          float* ssum, float* partial, unsigned* counter, void* stream);
int pf_couple_inject2_bwd(const float* out, const float* dout, const float* dssum, const float* s, int td, long long R,
                          float* dy, float* dobuf, float* ds, float* dt, void* stream);
int pf_inject_inv2_fwd(const float* u, const float* s, const float* t, int Rr, long long R, float* v, void* stream);
int pf_inject_inv2_bwd(const float* u, const float* s, const float* dv, int Rr, long long R, float* du, float* ds, float* dt,
                       void* stream);

/* out = ((p0 + p1) + p2) + ... for n_terms in 2..8 tensors of n floats each (n % 4 == 0, 16-byte aligned): the gradient of a
 * tensor with several consumers in ONE launch instead of autograd's n_terms - 1 pairwise adds (train_ops.FanoutFn).  ptrs: host
 * array of device pointers.  `out` may be one of the operands. */
int pf_sum_n(const float* const* ptrs, int n_terms, float* out, long long n, void* stream);

/* n <= 8 contiguous device regions of 32-bit words (4-byte aligned), dst[j][0 .. words[j]) = src[j][...], in ONE launch: the
 * batch of a captured training step into the tensors its graph reads (train_graph.GraphedTrainStep).  src / dst / words: host
 * arrays. */
int pf_copy_n(const void* const* src, void* const* dst, const long long* words, int n, void* stream);

/* WeightEstimationUnit's first conv folded into its producers' last linear layers (interpflow.py:98, 134, 144-146, 219-221: no
 * nonlinearity between them): W0 = [W0a | W0b] [o, 2 o], W6 [o, k6], Wout [o, ko]  ->  W6f = W0a W6, b6f = W0a b6 + b0,
 * Wof = W0b Wout, bof = W0b bout; _bwd: the chain rule from the gradients of those four back to W0, b0, W6, b6, Wout, bout.
 * Tiny, fixed summation order (bit-reproducible), one launch each. */
int pf_fold_wu_fwd(const float* W0, const float* b0, const float* W6, const float* b6, const float* Wout, const float* bout,
                   int o, int k6, int ko, float* W6f, float* b6f, float* Wof, float* bof, void* stream);
int pf_fold_wu_bwd(const float* W0, const float* W6, const float* b6, const float* Wout, const float* bout, int o, int k6, int ko,
                   const float* dW6f, const float* db6f, const float* dWof, const float* dbof, float* dW0, float* db0,
                   float* dW6, float* db6, float* dWout, float* dbout, void* stream);

/* ---- fused glue of the training step (csrc/train_glue.hip): what were chains of one-element torch launches ----
 * pf_interp_wsum: interpolation of the latent (modules/discrete/interpflow.py:153-186, 312-318): softmax over the K = 8
 *   neighbours of the first R <= 8 weight channels of w [T, 8, ldw] and the weighted sum of the gathered latent rows
 *   z [B N, 3] (idx [T, 8] batch-local), written as the [T R, 3] rows flow g reads; a [T, 8, R] is kept for the backward,
 *   which returns dw [T, 8, ldw] and dz [B N, 3] (zero-filled, then scatter-added with float atomics).
 * pf_emd_init: inputs of the auction (metric/emd/emd_module.py:45-56): price = 0, assignment = assignment_inv = -1.
 * pf_pugan_loss: train_pugan.py:52-67, out[0] = w_logp logp + w_emd sum_b sum_n dist[b,n] / radius[b] + w_cd mean_b per[b],
 *   out[1..3] = the weighted EMD, logp and CD terms (per nullable: the EMD-only mix of train_pu1k.py:62-67); backward: the seeds graddist [B,N] (pf_emd_backward), g1 [B,N], g2 [B,M]
 *   (pf_chamfer_bwd), dlogp [1] and the zero-filled gx [B,N,3], gy [B,M,3] those kernels accumulate into. */
int pf_interp_wsum_fwd(const float* w, int ldw, const float* z, const int* idx, int N, int K, int R, long long T, float* a,
                       float* u, void* stream);
int pf_interp_wsum_bwd(const float* a, const float* z, const int* idx, const float* du, int N, int K, int R, int ldw, long long T,
                       float* dw, float* dz, void* stream);
/* csr_off / csr_edge non-NULL (pf_knn_csr of idx): dz as a gather over the sorted transposed lists instead of float atomics */
int pf_interp_wsum_bwd_det(const float* a, const float* z, const int* idx, const float* du, int N, int K, int R, int ldw, long long T,
                       float* dw, float* dz, const int* csr_off, const int* csr_edge,
                           void* stream);
int pf_emd_init(float* price, int* assign2, long long Bn, void* stream);
int pf_pugan_loss_fwd(const float* logp, const float* dist, const float* radius, const float* per, int B, int n, float w_logp,
                      float w_emd, float w_cd, float* out, void* stream);
int pf_pugan_loss_bwd(const float* g, const float* radius, int B, int N, int M, float w_logp, float w_emd, float w_cd,
                      float* graddist, float* g1, float* g2, float* dlogp, float* gx, float* gy, void* stream);
/* The prediction's gradient of the same loss in two launches instead of four (pf_pugan_loss_bwd + pf_chamfer_bwd + pf_emd_backward:
 * train_pugan.py:52-67, emd_cuda.cu:284-300, metric/loss.py:39-42): g [1] = d loss, x [B,n,3] prediction, y [B,n,3] ground truth,
 * assign [B,n] the auction's assignment, idx1 / idx2 [B,n] Chamfer's nearest neighbours (both NULL: no Chamfer term), radius [B]
 * nullable -> gx [B,n,3] (own terms stored, the second Chamfer direction added with float atomics), dlogp [1] = g w_logp.  No
 * gradient for y. */
int pf_pugan_grad(const float* g, const float* radius, const float* x, const float* y, const int* assign, const int* idx1,
                  const int* idx2, int B, int n, int m, float w_logp, float w_emd, float w_cd, float* gx, float* dlogp, void* stream);

/* ---- gradient clipping (L2 norm over all parameters) + Adam for the whole model in two launches (csrc/optim.hip) ----
 * Replaces torch.nn.utils.clip_grad_norm_ (Lightning gradient_clip_val, train_pu1k.py:149) + torch.optim.Adam.step
 * (train_pu1k.py:46).  flat_g / m / v: [numel] in the chunk table's flat layout; params: device array of parameter addresses;
 * chunks: device int32 [nchunks][4] = (tensor id, offset in the tensor, length, offset in the flat buffers), no chunk crosses
 * a tensor; lr, step: device scalars (step is incremented here, before use); partial: >= nchunks doubles; counter: one zero
 * word (left zero); coef: 4 floats - [0] clip coefficient, [1] gradient norm before clipping, [2] 1 when THIS update was skipped
 * because the norm is not finite (parameters, moments and the step counter untouched), [3] += 1 per skipped update (the caller
 * zeroes it). */
int pf_clip_adam(float* flat_g, float* m, float* v, float* const* params, const int* chunks, int nchunks, const float* lr,
                 float* step, float beta1, float beta2, float eps, float max_norm, double* partial, unsigned* counter,
                 float* coef, void* stream);
/* pf_clip_adam with the gradients where autograd left them: grads = device array of nparams gradient addresses in the chunk
 * table's tensor order (contiguous fp32, one per parameter; point a parameter without gradient at zeros) instead of one flat
 * buffer - no concatenation launch in front of the update.  The clipped gradients are written back through the table. */
int pf_clip_adam_ptrs(float* const* grads, float* m, float* v, float* const* params, const int* chunks, int nchunks, const float* lr,
                      float* step, float beta1, float beta2, float eps, float max_norm, double* partial, unsigned* counter,
                      float* coef, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Patch pipeline around the network (modules/utils/patch.py:35-214), csrc/patch_ops.hip
 * ------------------------------------------------------------------------------------------- */

/* Farthest point sampling.  Replaces pointnet2_ops furthest_point_sample (patch.py:102,156).
 * xyz [B,N,3] -> idx_out [B,npoint] int32; starts at index 0; first maximum wins ties; mind: [B,N] float scratch,
 * 8-byte aligned (running min-distances, or - clouds of >= 8192 points, <= 32 cooperating workgroups per cloud -
 * the candidate exchange ring; overwritten either way). */
int pf_fps(const float* xyz, int B, int N, int npoint, float* mind, int* idx_out, void* stream);
/* the same samples (bit for bit) with a layout hint: group > 0 = every `group` consecutive points are one spatial neighbourhood
 * (PatchHelper.merge_pc, modules/utils/patch.py:142-165: the candidates arrive patch after patch, 256 x (upratio + 1) each).  For
 * group = 768 / 1280 / 1536 a wave of the cooperative kernel then holds exactly one neighbourhood, whose bounding box lets it skip
 * the samples that cannot reach it.  group = 0 or any other value: pf_fps. */
int pf_fps_grouped(const float* xyz, int B, int N, int npoint, int group, float* mind, int* idx_out, void* stream);

/* Layout of pf_fps's scratch when the cooperative kernel runs (return value 1; 0 = single-workgroup kernel, no ring):
 * cloud b's ring starts at 64-bit word b * stride_words of `mind`; word `abort_word` of a ring is the cloud's status after
 * the launch: 0 = every step completed; 1 = its workgroups gave up waiting for each other (bounded spin); 2 = it never
 * finished (or never got its workgroups).  Non-zero = that cloud's idx_out row is invalid.  Word abort_word + 1 holds the
 * number of exchange rounds the cloud took (two-sample kernel: npoint / rounds samples per round; measurement only). */
int pf_fps_scratch_layout(int N, long long* stride_words, long long* abort_word);

/* Measurement aid (bench.py --mode pugan): `rounds` rounds of the cooperative FPS kernel's candidate exchange between G
 * workgroups (2..32) with no points to update - the latency floor of one round of pf_fps's cooperative kernel.  ring: >= 1032
 * 64-bit words of scratch; ring[1024] == 0 afterwards when every round completed.  No reference counterpart. */
int pf_fps_exchange_probe(int G, int rounds, unsigned long long* ring, void* stream);

/* PatchHelper.normalize_pc (modules/utils/patch.py:168-178): centroid = mean over the N points, x - centroid, divided by the
 * largest norm.  x, out [B,N,3] (out may alias x), centroid [B,3], fdist [B].  One workgroup per cloud with a fixed
 * summation order: a cloud's result does not depend on B. */
int pf_normalize_pc(const float* x, int B, int N, float* out, float* centroid, float* fdist, void* stream);

/* ---- ragged ("packed") forms of the patch operators: B clouds of n[i] points stored back to back as one [sum n, 3] array.
 * n, npoint, m are HOST arrays of B ints (the per-cloud tables travel to the kernels as launch arguments: nothing is uploaded,
 * nothing synchronises).  Contract: every cloud gets, bit for bit, what the dense entry point above gives it when it runs
 * alone (B = 1); a cloud's result depends on no other cloud of the batch. */
/* pf_normalize_pc per cloud: out [sum n, 3] (may alias x), centroid [B,3], fdist [B]. */
int pf_normalize_pc_ragged(const float* x, const int* n, int B, float* out, float* centroid, float* fdist, void* stream);
/* Scratch of pf_fps_ragged for these sizes and this group hint (HOST function, no GPU work): scratch_off[i] = first float of
 * cloud i's row (even: a cooperative cloud's candidate ring is read there as 64-bit words), wgs[i] = workgroups cloud i gets
 * in the cooperative launch (0 = fewer than 8192 points: single-workgroup kernel), total_floats = size of the scratch array;
 * cloud i's status word is the 64-bit word status_word + i * status_stride of the scratch (values as pf_fps_scratch_layout:
 * 0 = complete; here EVERY cloud has one, whichever kernel ran it), followed by its exchange-round count.  All outputs
 * nullable.  Returns the points per thread of the cooperative launch (0: none needed) or a negative PF_ERR_* code. */
int pf_fps_ragged_layout(const int* n, int B, int group, long long* scratch_off, int* wgs, long long* total_floats,
                         long long* status_word, long long* status_stride);
/* pf_fps_grouped per cloud: npoint[i] <= n[i] samples of cloud i -> idx_out [sum npoint] int32 (indices inside the cloud).
 * scratch: pf_fps_ragged_layout's total_floats, 8-byte aligned.  At most two kernel families per pass - the cooperative one
 * for the clouds of >= 8192 points (one launch per 64 clouds: workgroups cloud-major in ascending order, G_i = wgs[i] each, so
 * in-order dispatch keeps every workgroup of the lowest unfinished cloud resident, as in pf_fps), one workgroup per cloud
 * for the others - with one points-per-thread shape per pass (chosen for the largest cloud; it changes no index). */
int pf_fps_ragged(const float* xyz, const int* n, const int* npoint, int B, int group, float* scratch, int* idx_out,
                  void* stream);
/* pf_fps_ragged with a fixed context (no reference counterpart; the merge of a tiled pass): ctx [sum n_ctx, 3]
 * holds, cloud after cloud, points that are already taken (n_ctx: HOST array of B ints >= 0; ctx may be null when all are 0).
 * Every candidate's running min-distance of cloud i starts as the smallest squared distance to its n_ctx[i] context points (the
 * same unfused arithmetic as the update); every sample, the first included, is then the arg-max (first maximum wins ties).
 * Context points are never output.  r2_out [B] (nullable): the min-distance cloud i's last sample had when it was taken (1e10
 * for a single sample without a context).  A cloud with n_ctx[i] = 0 gets pf_fps_ragged's samples bit for bit, starting at its
 * index 0, whatever the other clouds of the pass have.  Scratch, status words, group hint and launches as pf_fps_ragged. */
int pf_fps_ragged_ctx(const float* xyz, const int* n, const int* npoint, const float* ctx, const int* n_ctx, int B, int group,
                      float* scratch, int* idx_out, float* r2_out, void* stream);
/* pf_knn_large per cloud: ref [sum n, 3], query [sum m, 3] (m[i] queries against cloud i) -> idx_out [sum m, K] (indices
 * inside the cloud), dist_out [sum m, K] (nullable).  K <= every n[i]; clouds beyond 16384 points stream as in pf_knn_large. */
int pf_knn_large_ragged(const float* ref, const float* query, const int* n, const int* m, int B, int K, int* idx_out,
                        float* dist_out, void* stream);
/* pf_nn1 per cloud: p1 [sum n, 3] queries, p2 [sum m, 3] references -> dist_out [sum n], idx_out [sum n] (nullable). */
int pf_nn1_ragged(const float* p1, const float* p2, const int* n, const int* m, int B, float* dist_out, int* idx_out,
                  void* stream);

/* Text format of the CLI's output clouds (HOST memory, no GPU work): the bytes np.savetxt(path, cloud, fmt='%.6f') writes
 * (modules/discrete/upsample.py:57) - rows of c "%.6f" values separated by one blank, '\n' after every row.  pts [n,c]
 * float32; out must hold pf_format_xyz_bound(n, c) bytes.  Returns the bytes written or a negative PF_ERR_* code. */
long long pf_format_xyz_bound(long long n, int c);
long long pf_format_xyz(const float* pts, long long n, int c, char* out, long long cap);

/* Reader for the CLI's input clouds (HOST memory): the values np.loadtxt(path, dtype=np.float32) returns (upsample.py:42) for
 * whitespace-separated numeric text ('#' comments, blank lines skipped, double parse then rounded to float32).  text[len]
 * must be 0.  Returns the number of values written (rows x *ncols) or a negative PF_ERR_* code (UNSUPPORTED: a token that is
 * not a number - fall back to numpy; SHAPE: ragged rows; WORKSPACE: out too small). */
long long pf_parse_xyz(const char* text, long long len, float* out, long long cap, int* ncols);

/* K nearest references of every query for large K (patch extraction, K = 256).  Replaces knn_cuda.KNN
 * (patch.py:33,107).  ref [B,N,3], query [B,M,3], K <= N (any N; K <= 8192 when N > 16384: the references are then
 * streamed through LDS in chunks) -> idx_out [B,M,K] int32 ordered by (distance, index); dist_out [B,M,K] squared L2
 * (nullable). */
int pf_knn_large(const float* ref, const float* query, int B, int N, int M, int K, int* idx_out, float* dist_out,
                 void* stream);

/* ---------------------------------------------------------------------------------------------
 * Continuous (CNF) flow blocks (modules/continuous/), csrc/cnf.hip.  State rows are [y0 y1 y2 logp].
 * ------------------------------------------------------------------------------------------- */

/* One right-hand-side evaluation of a block's ODE, fused with the Runge-Kutta stage state:
 *   yi = y0 + h * sum_{j<ncoef} coef[j] * k[j]          (k: [7][rows][4] stage buffer; coef: host array)
 *   kout = sgn * ( f(t, yi), -e^T (df/dy) e )            (ODEfunc.forward odefunc.py:121-148, ODEnet :60-104,
 *                                                          ConcatSquashLinear diffeq_layers.py:72-86,
 *                                                          divergence_approx odefunc.py:9-31)
 * ctx [T,288]: per-point context terms (packing.pack_cnf_block), e [T,3] Hutchinson vector, row -> point = row / R,
 * rec: the block's weight record.  yout (nullable) receives yi.  sgn = -1 integrates backwards in time the way
 * torchdiffeq does (t' = -t, f' = -f). */
int pf_cnf_rhs(const float* y0, const float* k, const float* coef, int ncoef, float h, float t, float sgn,
               const float* ctx, const float* e, const float* rec, float* kout, float* yout, int rows, int R,
               void* stream);

/* Vector-Jacobian product of that right-hand side (csrc/cnf_bwd.hip), the kernel a differentiable flow block is built on.
 * With k = sgn * ( f(t, y), -e^T (df/dy) e ) - pf_cnf_rhs's kout for the state y [rows,4] - and S = sum_rows kbar . k:
 *   ybar   [rows,4]  OVERWRITTEN  dS/dy, column 3 zero (log p never enters f)
 *   ctxbar [T,288]   +=           dS/d(hyper-network outputs) per original point, summed over the point's R rows, in the ctx
 *                                 layout gate1[64] bias1[64] gate2[64] bias2[64] gate3 bias3.  In the units of the model's own
 *                                 pre-activations (the -log2e / 2 log2e the forward folds into ctx are NOT in it), and layer 3
 *                                 uses the first of its four replicated slots only: columns 256..258 and 272..274; the
 *                                 columns 259..271 and 275..287 are never touched.
 *   grad   [4900]    +=           [0,4096) dW2 [64][64]   [4096,4288) dW1 [64][3]   [4288,4352) db1   [4352,4416) db2
 *                                 [4416,4608) dW3 [3][64]   [4608,4611) db3   [4611] unused
 *                                 [4612,4900) gradients of the 288 time coefficients, ctx layout as for ctxbar: t x the column
 *                                 sums of THIS evaluation's ctxbar contributions (not recoverable from ctxbar later, which
 *                                 sums evaluations taken at different t).  All in the parameters' own units.
 * rows must be a multiple of R and R <= 16: a 16-row MFMA tile holds floor(16 / R) whole points, so a point never straddles
 * tiles and its rows are summed inside the wave.  No float atomics: workgroups sum their tiles on chip, write one partial slab
 * each into ws, and a second small launch adds the slabs in a fixed order - results are the same bits from run to run.
 * ws: pf_cnf_rhs_vjp_workspace_bytes(rows, R) bytes (negative: bad shape), never more than 256 * 4900 floats. */
long long pf_cnf_rhs_vjp_workspace_bytes(int rows, int R);
int pf_cnf_rhs_vjp(const float* y, const float* kbar, float t, float sgn, const float* ctx, const float* e, const float* rec,
                   float* ybar, float* ctxbar, float* grad, int rows, int R, void* ws, void* stream);

/* The reverse sweep of n_steps recorded Dormand-Prince steps in ONE launch (+ one slab reduction): what 6 n_steps calls of
 * pf_cnf_rhs_vjp, the stage recomputation by pf_cnf_rhs and the pf_lincomb combinations between them compute, with the step
 * sizes as constants.  Per step, last to first: the stage states Y_1 .. Y_6 are recomputed from the step's start (FSAL is an
 * ordinary dependence on it), then for j = 6 .. 1
 *   kbar_j = h b_j y1bar + h sum_{m > j} a_mj Ybar_m,   Ybar_j = VJP_F(Y_j, sgn (s + alpha_j h); kbar_j),
 * and y0bar = y1bar + sum_j Ybar_j is the cotangent the step before starts from (column 3 passes through: log p never enters f).
 *   states [n_steps, rows, 4]  the state at the START of each accepted step, forward order
 *   steps  [n_steps, 2]        DEVICE floats (s, h) in solver time, the fp32 values the forward was given (pf_cnf_steps_taped
 *                              writes both arrays)
 *   ybar   [rows,4]            in: the cotangent of the final state; out: the cotangent of states[0]
 *   ctxbar, grad               +=, layout and units of pf_cnf_rhs_vjp; every evaluation's share of the 288 time-coefficient
 *                              gradients carries that evaluation's own net time
 * A workgroup keeps a 64-row tile's stage states and cotangents in LDS and its weight-gradient sums in registers over all
 * stages, steps and tiles, and writes one slab: no grid barrier, no float atomics, the same bits from run to run.
 * rows, R, ws: as pf_cnf_rhs_vjp (the workspace sizes are equal); n_steps >= 1. */
long long pf_cnf_tape_vjp_workspace_bytes(int rows, int R);
int pf_cnf_tape_vjp(const float* states, const float* steps, int n_steps, float sgn, const float* ctx, const float* e,
                    const float* rec, float* ybar, float* ctxbar, float* grad, int rows, int R, void* ws, void* stream);

/* The forward counterpart of pf_cnf_tape_vjp: n_steps Dormand-Prince steps on a step list given IN ADVANCE (a frozen schedule)
 * in ONE launch, no controller.  On a fixed list nothing couples the rows, so a lane carries its row's state, its seven stage
 * derivatives and its Hutchinson vector through all steps in registers: k_1 = f(s_0, y_0) is evaluated here, after that FSAL.
 * The arithmetic is pf_cnf_init's f0 and pf_cnf_steps_taped's attempts (plain gates): on the list those recorded, the same bits.
 *   x       [rows, x_stride]        points, row stride 3 or 4 floats (a previous block's state is read in place); y_0 = (x, 0)
 *   steps   [n_steps, 2]            DEVICE floats (s, h) in solver time; reverse != 0: torchdiffeq's decreasing-time convention
 *                                   (net time = -s, f negated), as pf_cnf_steps_taped
 *   states  [n_steps + 1, rows, 4]  nullable: the state at the start of each step, then the result - the tape pf_cnf_tape_vjp reads
 *   y_out   [rows, 4]               the result
 *   f_start, f_end [rows, 4]        nullable: the derivative at the start of the first and at the end of the last step
 *   errsq   [n_steps]               nullable DEVICE doubles: per step sum_i (err_i / (atol + rtol max(|y0_i|, |y1_i|)))^2 of the
 *                                   embedded error estimate, the sum an adaptive attempt hands its controller.  Every wave
 *                                   keeps its share per step in ws and a second small launch adds the shares in a fixed order:
 *                                   no float atomics, the same bits from run to run.  ws: pf_cnf_replay_workspace_bytes(rows,
 *                                   n_steps) bytes (negative: bad shape); not read when errsq is NULL.
 * n_steps >= 1, x_stride 3 or 4, R >= 1, rows a multiple of R, else PF_ERR_SHAPE before anything is launched.  At most 1024
 * workgroups, grid-striding over 64-row tiles; for R >= 4 dividing 64 a tile's context rows are in LDS for all 6 n_steps + 1
 * evaluations.  No grid barrier, no controller word, no residency requirement. */
long long pf_cnf_replay_workspace_bytes(int rows, int n_steps);
int pf_cnf_replay(const float* x, int x_stride, const float* steps, int n_steps, int reverse, const float* ctx, const float* e,
                  const float* rec, float* states, float* y_out, float* f_start, float* f_end, double* errsq, float rtol,
                  float atol, int rows, int R, void* ws, void* stream);

/* One whole Dormand-Prince 5(4) step attempt per launch (the six stage evaluations fused, stage derivatives in
 * registers): y1 = y0 + h sum b_j k_j with k_1 = f0 (FSAL), f1 = k_7, ymid (nullable) = dense-output mid-point,
 * out[0] (double, device) = sum_i (err_i / (atol + rtol max(|y0_i|, |y1_i|)))^2 of the embedded error estimate.
 * t = start of the step in solver time; reverse != 0: torchdiffeq's decreasing-time convention (net time = -t, f negated).
 * ws: >= 1024 doubles.  Arithmetic of torchdiffeq's `_runge_kutta_step` / `_compute_error_ratio` called from cnf.py:97-113. */
int pf_cnf_step(const float* y0, const float* f0, float t, float h, int reverse, const float* ctx, const float* e,
                const float* rec, float* y1, float* f1, float* ymid, float rtol, float atol, int rows, int R, double* ws,
                double* out, void* stream);

/* ctx [T, 288] = c [T, cd] Hc^T + hb: the context's share of every gate / bias pre-activation of a flow block's three
 * ConcatSquash layers (modules/continuous/diffeq_layers.py:72-86), one split-fp16 GEMM (fp32-grade, bound by its 1 152-byte row
 * writes).  hc_image: Hc [288, cd] as the f16n fragment image of packing.pack_cnf_context, inv_scale: the inverse of the image's
 * power-of-two scale.  cd: 32, 64 or 128. */
int pf_cnf_context(const float* c, int cd, const float* hc_image, const float* hb, float inv_scale, float* ctx, int T, void* stream);

/* The weight records of nb <= 6 blocks from their LIVE parameter tensors, on the device, in one launch (csrc/cnf_pack.hip): what
 * packing.pack_cnf_block, pack_cnf_context and cnf_hyper_matrix make on the host, bit for bit.  A training step packs here: the
 * host packers cost a device -> host copy of every parameter and ~70 small uploads per block and call.
 *   params  HOST array of 16 nb DEVICE pointers (contiguous fp32), per block: for layer l = 0, 1, 2 of odefunc.diffeq.layers
 *           _layer.weight, _layer.bias, _hyper_gate.weight [out, 1 + cd], _hyper_gate.bias, _hyper_bias.weight [out, 1 + cd];
 *           then sqrt_end_time
 *   cd      HOST array [nb]: the context width of each block, 32, 64 or 128
 *   rec     [nb, 10160]   the weight records (csrc/pf_cnf.h: CNF_REC)
 *   hb      [nb, 288]     the context GEMM's bias (folded)
 *   hc, hplain, image     HOST arrays [nb] of DEVICE pointers to [288, cd[b]] floats each: the folded hyper matrix, the unfolded
 *           one (the backward of the context GEMM multiplies by it) and the f16n fragment image of hc x 2^sw for pf_cnf_context
 *   meta    [nb, 4] DEVICE doubles: [0] T_end = sqrt_end_time^2 (exact), [1] 2^-sw = pf_cnf_context's inv_scale, [2] status: bit 0
 *           an f16x2 image of the record, bit 1 the f16n image holds a magnitude >= 65504 (the host packers raise ValueError
 *           there; the outputs of such a block are not to be used), [3] zero.  The caller reads it once for all blocks.
 * No grid barrier, no atomics, no residency requirement. */
int pf_cnf_pack_blocks(const float* const* params, const int* cd, int nb, float* rec, float* hb, void* const* hc,
                       void* const* hplain, void* const* image, double* meta, void* stream);

/* n_attempts dopri5 step attempts with the step-size controller ON THE DEVICE (no host read between attempts).
 * ctl: 16 doubles - [0] t [1] dt [2] t1 [3] n_tot (elements of the RMS norm) [4] cur (which of ya / yb, fa / fb is current)
 * [5] done [6] accepted [7] rejected [8] nfe [9] status (0 ok, 1 non-finite error norm, 2 dt underflow) [10] reverse.
 * The host initialises ctl and the current buffers, enqueues batches and reads `done` once per batch; `out` [rows,4] holds
 * the state at t1 when done with status 0.  ws: >= 1024 doubles.
 * flags: PF_CNF_SPLIT_GATES - the caller vouches that log2(e) x max|t-column of the three hyper_gate weights| x |t1 - t0| <= 100
 * for this record (packing.cnf_split_ok).  The gates' 2^(gt (t + alpha h) + gc) then factor, without overflow, into a part per
 * point and step and a part per channel and stage: 36 of an evaluation's 135 transcendental instructions less. */
#define PF_CNF_SPLIT_GATES 1
int pf_cnf_steps(double* ctl, float* ya, float* yb, float* fa, float* fb, const float* ctx, const float* e, const float* rec,
                 float* out, float rtol, float atol, int rows, int R, int n_attempts, double* ws, int flags, void* stream);

/* pf_cnf_steps for an integration that pf_cnf_tape_vjp differentiates: the same controller state and batches of attempts, but
 *   - the states go to a tape: states [cap + 1, rows, 4], the state at the start of accepted step k in states[k] (pf_cnf_init
 *     writes states[0]); only fa / fb ping-pong;
 *   - an accepted step is recorded, steps [cap, 2] = (s, h): the fp32 values the kernel computed with.  The time advances in
 *     that arithmetic, s' = s + h in fp32, so the list is contiguous bit for bit;
 *   - the step that would cover t1 is cut to END there (h = t1 - t): no dense output, the result is states[ctl[6]];
 *   - status (ctl[9]) 3: cap steps are recorded and t1 is not reached - start again with a larger tape;
 *   - plain gates (no PF_CNF_SPLIT_GATES): the arithmetic the sweep recomputes. */
int pf_cnf_steps_taped(double* ctl, float* states, float* steps, int cap, float* fa, float* fb, const float* ctx, const float* e,
                       const float* rec, float rtol, float atol, int rows, int R, int n_attempts, double* ws, void* stream);

/* The start of that integration over [t0, t1] on the device, in two launches: the state rows y = (x, 0) from the points x
 * (row stride x_stride = 3 or 4 floats - a previous block's [rows,4] state is read in place), f0 = f(t0, y), ctl reset,
 * torchdiffeq's `_select_initial_step` into ctl[1].  n_tot: elements of the RMS norm; extra_d0 (DEVICE double, nullable)
 * x extra_scale: what the state rows outside y add to |y0 / scale|^2 (the context: pf_scaled_sumsq(c, NULL, c, ...)); no host
 * read anywhere in an integration's start.  ws: >= 3072 doubles.  ctl: ALL ZERO before its first use (every launch leaves its arrival word,
 * ctl[13], zero again). */
int pf_cnf_init(double* ctl, const float* x, int x_stride, float* y, float* f0, const float* ctx, const float* e,
                const float* rec, double t0, double t1, double n_tot, const double* extra_d0, double extra_scale, int reverse,
                float rtol, float atol, int rows, int R, double* ws, void* stream);

/* ---- a taped integration WITHOUT a look at its controller (the deferred training forward): pf_cnf_init_dev, ONE
 * pf_cnf_steps_taped call of as many attempts as the integration is expected to need (attempts after `done` return at once),
 * pf_cnf_tape_close; backward by pf_cnf_tape_vjp_dev.  The host reads the controller rows and the sticky table when it likes.
 *
 * pf_cnf_tape_close: the integration is CLEAN when ctl[5] != 0 and ctl[9] == 0.  Clean: y_out [rows,4] = states[(int)ctl[6]],
 * f_end [rows,4] = (ctl[4] ? fb : fa) - the result and the derivative at the end, at addresses that do not depend on the step
 * count.  Otherwise (attempts ran out, status 1 / 2, status 3 = tape full) both are filled with quiet NaN.
 *   sticky [4] ints, zero before the first use, never cleared by a launch: [0] runs, [1] runs that were not clean, [2] the last
 *   non-zero status, 4 = the attempts ran out, [3] the largest accepted + rejected count seen.  One lane, ordinary stores. */
int pf_cnf_tape_close(const double* ctl, const float* states, int cap, const float* fa, const float* fb, int rows, float* y_out,
                      float* f_end, int* sticky, void* stream);

/* pf_cnf_tape_vjp with the step count on the device: n = (int)ctl[6], read once per workgroup.  states [cap + 1, rows, 4] and
 * steps [cap, 2] are the whole tape.  A clean integration with 1 <= n <= cap gives the bits of pf_cnf_tape_vjp(.., n, ..).
 * Otherwise the kernel runs zero steps: ybar passes through, ctxbar and grad get nothing added (the slabs are written as zeros,
 * so the reduction reads initialised memory). */
int pf_cnf_tape_vjp_dev(const float* states, const float* steps, const double* ctl, int cap, float sgn, const float* ctx,
                        const float* e, const float* rec, float* ybar, float* ctxbar, float* grad, int rows, int R, void* ws,
                        void* stream);

/* pf_cnf_init over [0, T] (reverse: [-T, 0]) with T = t_end[0], a DEVICE double: word 0 of a pf_cnf_pack_blocks meta row. */
int pf_cnf_init_dev(double* ctl, const float* x, int x_stride, float* y, float* f0, const float* ctx, const float* e,
                    const float* rec, const double* t_end, double n_tot, const double* extra_d0, double extra_scale, int reverse,
                    float rtol, float atol, int rows, int R, double* ws, void* stream);

/* pf_cnf_context with inv_scale = scales[6], a DEVICE float (a row of pf_cnf_pack_status). */
int pf_cnf_context_dev(const float* c, int cd, const float* hc_image, const float* hb, const float* scales, float* ctx, int T,
                       void* stream);

/* Behind pf_cnf_pack_blocks, for a caller that never reads meta on the host: scales [nb, 8] floats, word 6 of row b = meta[b][1]
 * (pf_cnf_context_dev's argument).  A block with a non-zero status gets a record of NaN - every integration on it then ends with
 * status 1 - and sticky [4] ints (zero before the first use, never cleared here) latches it: [0] blocks seen, [1] blocks with a
 * status, [2] the last status, [3] its block. */
int pf_cnf_pack_status(const double* meta, int nb, float* rec, float* scales, int* sticky, void* stream);

/* out[i] = sum_{j<n_terms} w[j] * ptrs[j][i]   (n_terms <= 8; ptrs / w are HOST arrays).  Runge-Kutta solution,
 * mid-point and dense-output combinations of torchdiffeq's dopri5 (cnf.py:97-113 call site). */
int pf_lincomb(const float* const* ptrs, const float* w, int n_terms, float* out, long long n, void* stream);

/* out[0] (double, device) = sum_i (v_i / (atol + rtol * max(|s0_i|, |s1_i|)))^2, v = a - b (b, s1 nullable), or
 * v = h * sum_j w[j] * k[j][i] when n_terms > 0 (the embedded error estimate).  ws: >= 256 doubles.  Deterministic. */
int pf_scaled_sumsq(const float* a, const float* b, const float* s0, const float* s1, const float* k, const float* w,
                    int n_terms, float h, float rtol, float atol, long long n, double* ws, double* out, void* stream);

/* ---- evaluation metrics (csrc/eval_metrics.hip; the reference's scoring step, evaluation/evaluate.py) ---------------------- */

/* Approx-match EMD (Fan et al.; evaluation/tf_ops/approxmatch): the multi-level soft assignment of xyz1 [B,n,3] to
 * xyz2 [B,m,3] for levels -4^j, j = top .. -1, then 0, and cost[b] = sum_kl w_kl |a_k - b_l| / n (evaluate.py:59-65).
 * top = 7 is the CUDA op's schedule (the published numbers), 8 the CPU op's.  The match matrix is never stored: three sweeps
 * per level recompute it.  Deterministic, and a cloud's result does not depend on B.  top in [-2, 15], n, m <= 2^22, B <= 65535.
 * ws: pf_approxmatch_ws_floats(B, n, m, top) floats, 8-byte aligned. */
long long pf_approxmatch_ws_floats(int B, int n, int m, int top);
int pf_approxmatch_emd(const float* xyz1, const float* xyz2, int B, int n, int m, int top, float* cost, float* ws,
                       long long ws_floats, void* stream);

/* Point-to-mesh distance (evaluation/evaluation_code/evaluation.cpp:224-232, CGAL's AABB-tree closest point): dist[P] = the
 * Euclidean distance of every point of pts [P,3] to the closest point of the triangle soup tris [F,9] (v0 v1 v2), face[P]
 * (nullable) the index of that triangle (first minimum).  Exact closest point per triangle; the search prunes tiles of 64
 * consecutive triangles by their boxes, so points and triangles in a spatially coherent (Morton) order make it fast - any
 * order gives the same result.  seed [P] (nullable): a triangle index near each point's closest one (an upper bound to
 * start from).  brute != 0: no pruning (the baseline the pruned search equals).  ws: pf_point_mesh_ws_floats(P, F) floats. */
long long pf_point_mesh_ws_floats(int P, int F);
int pf_point_mesh_dist(const float* pts, int P, const float* tris, int F, const int* seed, int brute, float* dist, int* face,
                       float* ws, long long ws_floats, void* stream);

/* The same closest triangle over a uniform grid of the triangles (csrc/tri_grid.hip): for the same
 * pts [P,3], tris [F,9] and seed (nullable, same meaning and same default), dist[P] and face[P] (nullable) equal, BIT FOR BIT,
 * what pf_point_mesh_dist(..., brute = 1, ...) returns - including its tie rule: if the 64-triangle seed window attains the
 * minimal fp32 squared distance the winner is the window's first minimiser, otherwise the lowest triangle index attaining that
 * distance; dist is the winner's distance again in double, sqrt, cast to float.  The arithmetic is shared (csrc/pf_tri.h).
 *   Grid      the fp32 box of all triangle vertices; g = the smallest integer with g^3 >= 2 F, at most 256, cells along the
 *             longest extent, the same edge h on every axis (h >= 2^-19 of the largest |coordinate|, > 0), G_a = cell_a(hi_a) + 1
 *             cells on axis a (a zero-extent axis: one; all vertices coincident: G = (1, 1, 1)); cell_a(x) =
 *             clamp((int)floorf((x - lo_a) * (1 / h)), 0, G_a - 1) in unfused fp32, monotone in x.  A triangle is registered in
 *             EVERY cell its bounding box touches (conservative: no triangle-box test); one whose box touches more than 64
 *             cells goes to the oversize list instead, which every query tests after the seed window (a mesh of huge faces
 *             only degenerates to brute force; exactness is never affected).
 *   Search    one wave per query: the seed window, the oversize list, then the Chebyshev rings r = 0, 1, .. of cells around the
 *             query's (clamped) cell - queries outside the box are legal.  After ring r every unseen triangle lies wholly beyond
 *             a face of the visited block; the search stops when the squared gap to the nearest such face exceeds
 *             best (1 + 2^-12) + sc^2, sc = 2^-19 x the largest coordinate magnitude of query and box (pf_point_mesh_dist's
 *             margin for its boxes: the fp32 triangle distance is not correctly rounded), never on equality, and at the latest
 *             when the block covers the grid.  A query D cells from the surface visits on the order of D^3 cells: the search is
 *             meant for points near the surface; far queries are slow, never wrong.
 *   Calls     pf_point_mesh_grid_count builds the grid's histogram in ws (>= pf_point_mesh_grid_ws_bytes(P, F, 0) bytes) and
 *             writes info [8] (DEVICE, 64-bit): the (cell, triangle) pairs, the oversize triangles, G_x, G_y, G_z, and the byte
 *             offsets in ws of the cells' first pair positions (int [cells + 1], x fastest), of the oversize list and of the
 *             pair list.  The caller reads the pair count, sizes ws by pf_point_mesh_grid_ws_bytes(P, F, pairs) and calls
 *             pf_point_mesh_grid with that `pairs`, which builds the grid again and searches.  A ws sized for fewer pairs than
 *             the mesh has is safe: the pair list is not used then and every query scans all triangles.  More pairs than an
 *             int holds: PF_ERR_UNSUPPORTED from the size call.  P <= 2^26, F <= 2^28; ws 16-byte aligned.
 *   cand      (nullable) [P]: triangle evaluations per query - seed window, oversize list and rings.
 * No float atomics; integer atomics in the grid build only (the order inside a cell cannot show); every loop bounded by a
 * constant or a host-given size; every index read from a list is clamped before it addresses memory. */
long long pf_point_mesh_grid_ws_bytes(int P, int F, long long pairs);
int pf_point_mesh_grid_count(const float* tris, int F, void* ws, long long ws_bytes, long long* info, void* stream);
int pf_point_mesh_grid(const float* pts, int P, const float* tris, int F, const int* seed, float* dist, int* face, int* cand,
                       void* ws, long long ws_bytes, long long pairs, void* stream);

/* ---- training batches on the device (csrc/data_aug.hip; the reference's dataset/pu1k/fetcher.py:69-101) ---------------------
 * One launch assembles and augments rows [0, b) of a batch from a device-resident dataset: one workgroup per patch, no grid
 * barrier, no float atomics, no host synchronisation, no global state.
 *   inp [M, n_in, 3], gt [M, n_out, 3], radius [M] fp32; order [M] int32, a permutation of 0..M-1 (the epoch's shuffle).
 *   Row r takes patch order[(pos + r) mod M]; its random numbers belong to the GLOBAL PATCH SLOT slot0 + r (the caller passes
 *   step * batch_size + first row, so a rank that produces rows [lo, hi) of a batch gets exactly those rows of the whole batch).
 * Stages, in the reference's order, each behind its flag:
 *   PF_PATCH_SUBSAMPLE  n_in > n only: nonuniform_sampling - loc ~ U(0.1, 0.9), candidates int((loc + 0.3 z_j) n_in) (truncation),
 *                       out-of-range ones dropped, the first n DISTINCT ones in stream order kept (what the reference's
 *                       sequential rejection loop yields).  Candidates come in rounds of 1024, at most PF_PATCH_MAX_ROUNDS;
 *                       a patch still short then sets PF_PATCH_ST_SHORT and repeats its last index.  Needs
 *                       n_in <= PF_PATCH_MAX_NIN and n <= PF_PATCH_MAX_N (LDS tables), else PF_ERR_UNSUPPORTED.
 *                       n_in > n without this flag: PF_ERR_SHAPE.
 *   PF_PATCH_JITTER     input only: x += clip(sigma z, -clip, clip), three normals per point.
 *   PF_PATCH_ROTATE     input and gt: row vector times R = Rz Ry Rx, angles 2 pi u each; with PF_PATCH_Z_ROTATED R = Rz.
 *   PF_PATCH_SCALE      input, gt and radius times s ~ U(scale_low, scale_high).
 *   PF_PATCH_SHIFT      input and gt plus t ~ U(-shift_range, shift_range)^3; off when shift_range == 0.
 *   With no flag the outputs are copies of the selected patches (the validation setting).
 * Random numbers: Philox-4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 *   (element, stream, slot & 0xffffffff, slot >> 32), giving four 32-bit words x0..x3 per counter:
 *   stream 0 (parameters): element 0 -> x0: loc, x1 x2 x3: the angles about x, y, z; element 1 -> x0: scale, x1 x2 x3: shifts;
 *   stream 1 (candidates): stream position p reads element p / 4, words (x0, x1) for p mod 4 < 2, else (x2, x3);
 *                          z = r cos(2 pi u1) for even p, r sin(2 pi u1) for odd p, r = sqrt(-2 ln u0)   (Box-Muller);
 *   stream 2 (jitter):     point i of the OUTPUT reads element i: (x0, x1) -> the x and y noise (cos, sin), (x2, x3) -> z (cos).
 *   Word to uniform: u = (x >> 8) 2^-24 + 2^-25 in fp32, never 0; the one value that fp32 rounds to 1 is kept at 1 - 2^-24.
 *   U(lo, hi) = lo + (hi - lo) u; the shifts use 2u - 1 of the unrounded u (exact in fp32) times shift_range.
 *   logf, sinf, cosf are the precise ones; every operation is a separate fp32 rounding except the rotation, which is
 *   fma(z, R2j, fma(y, R1j, x R0j)) for output coordinate j - the same order for every row wherever it is produced.
 * Outputs: out_inp [b, n, 3], out_gt [b, n_out, 3], out_radius [b];
 *   params [b, 16], always written: R row-major (9; identity when off), scale (1 when off), shifts (3; 0 when off), loc (0 when
 *   no subsample), the number of candidate rounds drawn, 0;
 *   idx [b, n] (nullable): the index of inp's point behind every output point; cand [b, T] (nullable, tests): the candidate
 *   stream as drawn, out-of-range values included, positions < min(T, 1024 x rounds drawn) - the rest is left untouched;
 *   status: one int32 the kernel only ever ORs bits into (PF_PATCH_ST_*); the caller zeroes it once and reads it when it
 *   synchronises anyway. */
#define PF_PATCH_SUBSAMPLE 1
#define PF_PATCH_JITTER 2
#define PF_PATCH_ROTATE 4
#define PF_PATCH_Z_ROTATED 8
#define PF_PATCH_SCALE 16
#define PF_PATCH_SHIFT 32
#define PF_PATCH_ALL 63
#define PF_PATCH_MAX_NIN 8192
#define PF_PATCH_MAX_N 4096
#define PF_PATCH_MAX_ROUNDS 64
#define PF_PATCH_ST_SHORT 1     /* a patch had fewer than n distinct candidates after PF_PATCH_MAX_ROUNDS rounds */
#define PF_PATCH_ST_ORDER 2     /* order held a value outside [0, M): patch 0 was used instead                    */
int pf_patch_batch(const float* inp, const float* gt, const float* radius, const int* order, int M, int n_in, int n_out,
                   long long pos, int b, int n, unsigned long long slot0, unsigned long long seed, int flags,
                   float jitter_sigma, float jitter_clip, float scale_low, float scale_high, float shift_range,
                   float* out_inp, float* out_gt, float* out_radius, float* params, int* idx, int* cand, int T, int* status,
                   void* stream);

/* ---- uniformity of an upsampled cloud on its mesh (csrc/eval_uniform.hip; the reference's evaluate.py:105-165 analyze_uniform
 * and the disk search evaluation.cpp:79-113 was meant to feed it) --------------------------------------------------------------
 * Closest points: out[P,3] = the closest point of triangle face[p] of tris [F,9] to pts[p] (Voronoi-region classification in
 * double, relative to the point).  A face index outside [0, F) gives NaN, never a read outside tris. */
int pf_tri_closest_points(const float* pts, int P, const float* tris, int F, const int* face, float* out, void* stream);

/* Seeds on the surface: for s in [0, S) the words x0 x1 x2 of Philox-4x32-10 with key (seed & 0xffffffff, seed >> 32) and
 * counter (s, 0, 0, 0) give u0 u1 u2 (the word-to-uniform mapping above: never 0, never 1).  face[s] = the first f with
 * cum_area[f] > u0 cum_area[F-1] (cum_area [F] double, the running sum of the triangle areas - a device pointer; F - 1 when
 * there is none), seeds[s] = (1 - sqrt u1) a + sqrt u1 (1 - u2) b + sqrt u1 u2 c of that triangle, uniforms [S,3] = u0 u1 u2.
 * A seed depends on (mesh, seed, s) only.  S <= 2^24. */
int pf_mesh_sample(const float* tris, int F, const double* cum_area, int S, unsigned long long seed, float* seeds, int* face,
                   float* uniforms, void* stream);

/* Disks: the points of mapped [N,3] within the Euclidean distance radii[j] of seeds[s] (seeds [S,3]; radii [J] HOST doubles,
 * positive and ascending, J <= PF_DISK_MAX_RADII), |mapped - seed|^2 <= fp32(radii[j]^2) with the seed subtracted first.
 *   pf_disk_count: counts [S,J] int32.
 *   pf_disk_fill:  row s of the CSR, member / level [offsets[s], offsets[s+1]) (offsets [S+1] int64 on the device, sized by the
 *                  caller from counts[:, J-1]): the members of the largest disk in ascending index order and, for each, the
 *                  smallest j whose disk holds it.  A row shorter than its disk is filled and not overrun.
 * One workgroup per seed sweeps all N points; order comes from wave ballots and prefix counts, not from atomics. */
#define PF_DISK_MAX_RADII 8
int pf_disk_count(const float* mapped, int N, const float* seeds, int S, const double* radii, int J, int* counts, void* stream);
int pf_disk_fill(const float* mapped, int N, const float* seeds, int S, const double* radii, int J, const long long* offsets,
                 int* member, int* level, void* stream);

/* The statistic of every disk of a CSR (from pf_disk_fill or from files): member k of row s belongs to disk (s, j) when
 * level[k] <= j.  out_n [S,J] = the member count, out_dis [S,J] = mean over the members of (d - e)^2 / e, with d the distance
 * to the nearest OTHER member of the same disk (another entry of the row: duplicated points give 0) and
 * e = sqrt(2 (pi radii[j]^2 / n) / 1.732); NaN for fewer than two members.  Both double.  Squared distances are fp32 sums of
 * squared fp32 differences; d, the terms and their sum (a fixed order) are double.  Rows of any length: PF_DISK_TILE members
 * are staged at a time (pf_disk_tile() returns it).  Member indices are clamped to [0, N), the caller validates them. */
#define PF_DISK_TILE 1024
int pf_disk_tile(void);
int pf_disk_uniformity(const float* mapped, int N, const long long* offsets, const int* member, const int* level, int S,
                       const double* radii, int J, double* out_n, double* out_dis, void* stream);

/* ---- Surface-connected neighbourhoods (csrc/surface_reach.hip; the reference has no runnable counterpart: its disks were
 * meant to come from CGAL's geodesic distance, evaluation.cpp:88-107) ----------------------------------------------------------
 * For a source point src[s] on face src_face[s] of tris [F,9]: d2(f) = the squared distance from the source to the closest
 * point of triangle f (Voronoi-region classification in double relative to the source, rounded once to fp32; the distance to
 * the plane of a face the source all but lies in - its own - is summed without cancellation, pf_surface.h plane_d2), and the
 * bottleneck field b2(f) = min over face paths src_face = g0 .. gk = f of max_i d2(g_i), faces adjacent as the caller's CSR
 * face_adj_offsets [F+1] int64 / face_adj says (metrics.face_adjacency: a shared welded vertex).
 *   pf_reach_count: counts [S] int32 = the faces with d2 <= r2_stop[s], the candidates - a superset of the faces reachable
 *                   inside that ball.  A source whose own face is no candidate (or outside [0, F): never read) counts 0 and
 *                   sets PF_REACH_ST_START.
 *   pf_reach_fill:  row s of the CSR, rface / rd2 [offsets[s], offsets[s+1]) (offsets [S+1] int64 on the device, sized by the
 *                   caller from counts): the candidates in ascending face index with their d2.  Order comes from wave ballots
 *                   and prefix counts, not from atomics.  A row shorter than its candidates is filled and not overrun.
 *   pf_reach_relax: rb2 [nnz] = b2 of every candidate, +inf for one not reached through candidates.  One workgroup per source
 *                   sweeps b2(f) <- min(b2(f), max(d2(f), b2(g))) over the adjacent candidates g (found by binary search in
 *                   the sorted row; unsigned atomicMin on the fp32 bits) until a sweep lowers nothing.  Values only fall, each
 *                   is the bottleneck of a real path, and the end state is the least fixed point - b2 itself - whatever the
 *                   sweep order, the wave scheduling, S or the grid; a repeat gives the same bits.  Every finite value is exact:
 *                   a path of bottleneck <= r2_stop uses only faces with d2 <= r2_stop, all candidates.  Rows of at most
 *                   PF_REACH_LDS_FACES entries (pf_reach_lds_faces() returns it) are worked on in LDS, longer ones in rb2
 *                   itself, by the same device code.  At most row length + 1 sweeps, then PF_REACH_ST_ITER; no grid barrier,
 *                   no co-residency requirement.  sweeps [S] int32 (nullable): the sweeps each source took.  A row that does
 *                   not hold its source's face sets PF_REACH_ST_START, one that lists a face outside [0, F) (never a row of
 *                   pf_reach_fill) PF_REACH_ST_ROW; neither is relaxed, and the adjacency is not read for it: all +inf.
 *   pf_reach_point_d2: out [S,N] = max(|pts[i] - src[s]|^2, b2(pts_face[i])), the squared surface distance of every point
 *                   (fp32, the source subtracted first, as pf_disk_count); +inf for a point on a face the row does not hold.
 * status: one int32 the kernels only OR PF_REACH_ST_* into. */
#define PF_REACH_LDS_FACES 4096
#define PF_REACH_ST_START 1     /* a source's own face is not among its candidates: its row is empty            */
#define PF_REACH_ST_ITER 2      /* a row did not settle within its length + 1 sweeps (never seen: a defect)      */
#define PF_REACH_ST_ROW 4       /* pf_reach_relax was given a row that lists a face outside [0, F): left +inf    */
int pf_reach_lds_faces(void);
int pf_reach_count(const float* tris, int F, const float* src, const int* src_face, const float* r2_stop, int S, int* counts,
                   int* status, void* stream);
int pf_reach_fill(const float* tris, int F, const float* src, const int* src_face, const float* r2_stop, int S,
                  const long long* offsets, int* rface, float* rd2, int* status, void* stream);
int pf_reach_relax(const long long* offsets, const int* rface, const float* rd2, int F, const long long* face_adj_offsets,
                   const int* face_adj, const int* src_face, int S, float* rb2, int* sweeps, int* status, void* stream);
int pf_reach_point_d2(const float* pts, int N, const int* pts_face, const float* src, int S, const long long* offsets,
                      const int* rface, const float* rb2, float* out, void* stream);
/* pf_disk_count / pf_disk_fill with the surface distance: a point is in disk (s, j) when
 * max(|mapped - seed|^2, b2(mapped_face)) <= fp32(radii[j]^2), b2 from row s of the reach CSR (reach_offsets, rface, rb2) made
 * with seeds as sources and r2_stop >= fp32(radii[J-1]^2).  The same kernels and the same CSR format as the Euclidean pair. */
int pf_disk_count_reach(const float* mapped, int N, const float* seeds, int S, const double* radii, int J, const int* mapped_face,
                        const long long* reach_offsets, const int* rface, const float* rb2, int* counts, void* stream);
int pf_disk_fill_reach(const float* mapped, int N, const float* seeds, int S, const double* radii, int J, const int* mapped_face,
                       const long long* reach_offsets, const int* rface, const float* rb2, const long long* offsets, int* member,
                       int* level, void* stream);

/* ---- Poisson-disk point sets by weighted sample elimination (csrc/poisson.hip; Yuksel 2015 - the reference has no counterpart:
 * its training patches and test clouds came from PU-GAN's Meshlab preparation) ------------------------------------------------
 * A pool is s candidate points on a surface of area A, thinned to exactly m.  B pools are stored back to back as one
 * [sum s, 3] array, like the ragged patch operators, and under their contract: every pool gets, bit for bit, what it gets alone.
 * Parameters (HOST, double, rounded to fp32 once): with t = m / s,
 *   r_max = sqrt(A / (2 sqrt(3) m)),  r_min = r_max (1 - t sqrt(t)) 0.65,
 *   consts = { R2 = fp32((2 r_max)^2), inv = fp32(1 / (2 r_max)), lo = fp32(2 r_min) }.
 * pf_poisson_params: one pool's values (all outputs nullable); SHAPE unless 1 <= m <= s and 0 < A < 1e30.
 * pf_poisson_pools:  the table the device entry points read (a HOST array the caller uploads): pool b's first candidate
 *   (off), first output slot (out_off), constants, and path = 1 when pf_poisson_eliminate_wg takes it (s <= PF_POISSON_WG_MAX and
 *   flags without PF_POISSON_NO_WG), 0 when pf_poisson_rounds does.  Both paths return the same indices. */
#define PF_POISSON_WG_MAX 8192
#define PF_POISSON_MAX_TOTAL (1 << 30)
#define PF_POISSON_NO_WG 1
#define PF_POISSON_ST_DEGREE 1  /* a candidate has 65535 neighbours or more (the pool is far denser than its radius assumes) */
#define PF_POISSON_ST_WEIGHT 2  /* a weight left 32 bits: the kept set is not the sequential one                            */
typedef struct PfPoissonPool {
    int off, s, m, out_off;
    float R2, inv, lo;
    int path;
} PfPoissonPool;
typedef struct PfPoissonState { /* per pool, on the device; zeroed by pf_poisson_begin */
    unsigned long long tau;     /* the phase's threshold key: (w << 32) | (0xffffffff - index)                              */
    int k, done, phases, rounds, alive, pad;
} PfPoissonState;
int pf_poisson_params(double area, int s, int m, double* r_max, double* r_min, float* consts);
int pf_poisson_pools(const int* s, const int* m, const double* area, int B, int flags, PfPoissonPool* pools);

/* The neighbour graph.  i ~ j (i != j, same pool) when d2 < R2 with d2 = ((dx dx) + (dy dy)) + (dz dz), unfused fp32 (the kNN
 * kernels' rule).  Edge weight: d = sqrt(d2) correctly rounded, x = max(1 - max(d, lo) inv, 0), every operation a separate
 * fp32 rounding, x^8 by three squarings, q_ij = (uint32) rint(x^8 65536); w_i = sum_j q_ij, an integer.
 *   pf_poisson_degree: deg [sum s] int32, the neighbours of every candidate;
 *   pf_poisson_graph:  row i of the CSR, nbr / q [offsets[i], offsets[i+1]) (offsets [sum s + 1] int64 on the device, the
 *                      running sum of deg): the neighbours' indices INSIDE THE POOL, ascending, and their q; w [sum s] uint32.
 *                      A row shorter than its degree is filled and not overrun.
 * pools: the DEVICE copy of pf_poisson_pools' table, max_s / total: the largest and the summed s.  One thread per candidate
 * sweeps its pool through LDS tiles (s^2 pair tests per pool).  status: one int32 the kernels only OR PF_POISSON_ST_* into. */
int pf_poisson_degree(const float* pts, const PfPoissonPool* pools, int B, int max_s, long long total, int* deg, int* status,
                      void* stream);
int pf_poisson_graph(const float* pts, const PfPoissonPool* pools, int B, int max_s, long long total, const long long* offsets,
                     int* nbr, int* q, unsigned* w, int* status, void* stream);

/* The elimination.  Its result is the alive set of the sequential process "while more than m are alive: remove the alive i
 * with the largest key (w_i, smaller index first), subtract q_ij from every alive neighbour j" - ascending indices inside the
 * pool, keep [out_off, out_off + m).  It is computed in phases and rounds instead (csrc/poisson.hip's head):
 * a phase fixes tau = the (k+1)-th largest alive key, k = alive - m; a round removes at once every alive candidate above tau
 * and above all its alive neighbours; the phase ends when no alive key exceeds tau.  Integer atomics only, no grid barrier.
 *   pf_poisson_begin:        state [sum s] int32 = alive, st [B] zeroed.  w is consumed by the elimination.
 *   pf_poisson_eliminate_wg: the pools of path 1, one workgroup per pool, every round inside one launch.
 *   pf_poisson_rounds:       rounds round0 .. round0 + n_rounds - 1 of the pools of path 0, three launches a round (the pool's
 *                            bookkeeping and radix select of tau in one workgroup; pick; apply).  *unfinished (device int32) is
 *                            set to r + 1 by round r when a pool still had work in it: the caller reads it after a batch and
 *                            stops when it is not round0 + n_rounds.  Rounds after a pool is done cost it nothing but the launch.
 * st[b].phases / .rounds count what pool b took. */
int pf_poisson_begin(const PfPoissonPool* pools, int B, int max_s, long long total, int* state, PfPoissonState* st, void* stream);
int pf_poisson_eliminate_wg(const PfPoissonPool* pools, int B, const long long* offsets, const int* nbr, const int* q, unsigned* w,
                            int* state, PfPoissonState* st, int* keep, void* stream);
int pf_poisson_rounds(const PfPoissonPool* pools, int B, int max_s, long long total, const long long* offsets, const int* nbr,
                      const int* q, unsigned* w, int* state, PfPoissonState* st, int* keep, int round0, int n_rounds,
                      int* unfinished, void* stream);

/* ---- Tiled passes over large clouds (csrc/tiles.hip, puflow_amd/tiles.py; the reference has no counterpart) ------------------
 * Boxes: the points of pts [M,3] with lo <= p <= hi on every axis, boxes [T,6] = lo xyz, hi xyz (+-inf allowed, faces belong
 * to the box; a box with lo > hi is empty).
 *   pf_box_count: counts [T] int32.
 *   pf_box_fill:  row t of the CSR, member [offsets[t], offsets[t+1]) (offsets [T+1] int64 on the device, sized by the caller
 *                 from counts): the members in ascending index order.  A row shorter than its box is filled and not overrun.
 * One workgroup per box sweeps all M points; order comes from wave ballots and prefix counts, not from atomics. */
int pf_box_count(const float* pts, int M, const float* boxes, int T, int* counts, void* stream);
int pf_box_fill(const float* pts, int M, const float* boxes, int T, const long long* offsets, int* member, void* stream);
/* Cells: leaf [M] int32 = the leaf (0 .. 2^L - 1, left to right) every point of pts [M,3] reaches in a complete k-d tree of
 * depth L (0 <= L <= 24) given in heap order - inner node k splits axis[k] (0, 1, 2) at split[k], children 2k + 1 and 2k + 2,
 * 2^L - 1 inner nodes; a point goes right iff p[axis] >= split.  L = 0: every point is in leaf 0, axis / split are not read. */
int pf_kd_assign(const float* pts, int M, const int* axis, const float* split, int L, int* leaf, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-point attributes on the upsampled cloud (puflow_amd/attributes.py), csrc/attr.hip.  No reference
 * counterpart: the reference writes bare xyz.
 * ------------------------------------------------------------------------------------------- */
#define PF_ATTR_LIN 0           /* segment kind: weighted sum of the neighbours' values                    */
#define PF_ATTR_UNIT 1          /* 3 columns, a direction up to sign: sign-aligned, blended, normalised    */
#define PF_ATTR_NEAR 2          /* the nearest neighbour's values verbatim (labels)                        */
#define PF_ATTR_MAX_K 8
#define PF_ATTR_MAX_C 16
#define PF_NORMALS_MIN_K 8
#define PF_NORMALS_MAX_K 64

/* The columns a cloud carries beside xyz, moved to new points.  idx, d2 [B,M,K]: the K nearest of the cloud's N input points
 * of every output point, as pf_knn_large(ref = input, query = output) writes them (ordered by distance); attr [B,N,C] the input
 * points' rows; out [B,M,C].  The C columns are nseg consecutive segments, seg_kind[g] one of PF_ATTR_* over seg_cols[g]
 * columns (HOST arrays; the columns must add up to C, a UNIT segment has 3).  Weights w_k = (1 / d2_k) / sum_j (1 / d2_j), float32,
 * k = 0 .. K-1 in order, IEEE division.
 *   LIN   sum_k w_k attr_k
 *   UNIT  every neighbour's vector is negated when its dot product with neighbour 0's is negative, then blended as LIN and
 *         divided by its length; a length that is 0 or not finite writes neighbour 0's vector unchanged
 *   NEAR  neighbour 0's values
 * An output point with d2_0 == 0 (it IS an input point) gets neighbour 0's whole row bit for bit, whatever the plan.
 * 1 <= K <= PF_ATTR_MAX_K, 1 <= C <= PF_ATTR_MAX_C and a known kind, else PF_ERR_UNSUPPORTED; K <= N.  One launch. */
int pf_attr_blend(const int* idx, const float* d2, const float* attr, int B, int N, int M, int K, int C, const int* seg_kind,
                  const int* seg_cols, int nseg, float* out, void* stream);
/* pf_attr_blend per cloud of a ragged pass: attr [sum n, C], idx / d2 [sum m, K] (indices inside the cloud, as
 * pf_knn_large_ragged writes them), out [sum m, C]; n, m: HOST arrays of B ints.  Every cloud gets, bit for bit, what
 * pf_attr_blend gives it alone.  One launch per 64 clouds. */
int pf_attr_blend_ragged(const int* idx, const float* d2, const float* attr, const int* n, const int* m, int B, int K, int C,
                         const int* seg_kind, const int* seg_cols, int nseg, float* out, void* stream);
/* A normal per point from its own neighbourhood: pts [B,M,3], idx [B,M,K] from pf_knn_large(ref = query = pts) -> normal
 * [B,M,3] unit length, variation [B,M] = l0 / (l0 + l1 + l2) in [0, 1/3] (l0 <= l1 <= l2: eigenvalues of the neighbourhood's
 * covariance).  Centroid and centred second moments of the K neighbours in double, eigenvectors by 8 cyclic Jacobi sweeps in
 * double, the smallest eigenvalue's vector rounded to float32 once.  Sign: with viewpoint (HOST float[3], nullable)
 * dot(n, viewpoint - p) >= 0; without, dot(n, p - c) >= 0 for the cloud's centroid c, which this call writes to centroid [B,3]
 * (double, on the device; required without a viewpoint, not touched with one).  A neighbourhood whose moments are all 0 gets
 * (0, 0, 1) and variation 0.  PF_NORMALS_MIN_K <= K <= PF_NORMALS_MAX_K, else PF_ERR_UNSUPPORTED; K <= M. */
int pf_normals_pca(const float* pts, const int* idx, int B, int M, int K, const float* viewpoint, double* centroid,
                   float* normal, float* variation, void* stream);
/* pf_normals_pca per cloud of a ragged pass: pts [sum m, 3], idx [sum m, K] (pf_knn_large_ragged, indices inside the cloud),
 * m: HOST array of B ints.  Every cloud gets, bit for bit, what pf_normals_pca gives it alone. */
int pf_normals_pca_ragged(const float* pts, const int* idx, const int* m, int B, int K, const float* viewpoint, double* centroid,
                          float* normal, float* variation, void* stream);

/* ---- exact small-K nearest neighbours over a uniform grid (csrc/knn_grid.hip) -------------------------------
 * The same results as pf_knn_large / pf_knn_large_ragged, bit for bit - the K smallest keys (squared distance, index), the
 * squared distance the unfused fp32 ((dx*dx)+(dy*dy))+(dz*dz) - for 1 <= K <= PF_KNN_GRID_MAX_K, found by visiting
 * the cells of growing Chebyshev rings around the query's cell of a per-cloud uniform grid instead of sorting the whole cloud.
 * Shapes, index convention (indices inside the cloud), ordering and the nullable dist_out are pf_knn_large's.  Coordinates are
 * assumed finite.  ws: pf_knn_grid_ws_bytes(n, B) bytes of device memory, 16-byte aligned, rebuilt by every call (box, cells
 * and the cell-sorted references of each cloud); n / m: HOST arrays of B ints.  Before any device work: PF_ERR_NULL (ws too),
 * PF_ERR_SHAPE (B, N, M, n[i] or m[i] <= 0, K > N or K > any n[i], more than 2^31 / 3 points, misaligned ws),
 * PF_ERR_UNSUPPORTED (K outside 1 .. PF_KNN_GRID_MAX_K), PF_ERR_WORKSPACE (ws_bytes too small).  Five launches per 64 clouds,
 * integer atomics only, the same bits from run to run. */
#define PF_KNN_GRID_MAX_K 64
/* bytes of workspace for B clouds of n[i] references (pf_knn_grid: n[i] = N for all); negative PF_ERR_* on a bad argument */
long long pf_knn_grid_ws_bytes(const int* n, int B);
int pf_knn_grid(const float* ref, const float* query, int B, int N, int M, int K, void* ws, long long ws_bytes, int* idx_out,
                float* dist_out, void* stream);
int pf_knn_grid_ragged(const float* ref, const float* query, const int* n, const int* m, int B, int K, void* ws,
                       long long ws_bytes, int* idx_out, float* dist_out, void* stream);

/* ---- consistent signs for normals: propagation along a minimum spanning forest (csrc/normals_orient.hip) ------
 * pts, normal_in [B,M,3]; idx [B,M,K] as pf_knn_large(ref = query = pts) writes it (indices inside the cloud; an entry outside
 * the cloud is ignored).  normal_in may have any signs (pf_normals_pca's, a file's).
 *   Graph    the undirected edges {i, j}, i != j, with j in i's list or i in j's list.
 *   Weights  d_ij = ((nx_i*nx_j) + (ny_i*ny_j)) + (nz_i*nz_j) in unfused fp32 (bitwise symmetric), w_ij = max(0, 1 - |d_ij|) in
 *            fp32.  Edges are ordered by the key (w_ij, min(i,j), max(i,j)): a strict order, so the minimum spanning forest is
 *            unique whatever finds it.
 *   Signs    normal_out_i = normal_in_i with the sign bit of all three components flipped or not.  Along every forest edge i's
 *            flip differs from j's exactly when d_ij < 0 (d_ij == 0: no relative flip).  Per connected component the seed is
 *            the point with the largest z, or with viewpoint v (HOST float[3], nullable) the point with the smallest unfused
 *            fp32 squared distance ((dx*dx)+(dy*dy))+(dz*dz), d = p - v; the lowest index among equals.  The component as a whole
 *            is flipped or not so that the seed's output n' has n'_z >= 0, or with a viewpoint the unfused fp32
 *            ((n'x*(vx-px)) + (n'y*(vy-py))) + (n'z*(vz-pz)) >= 0; with an exact 0 the seed keeps its input sign.  A closed piece
 *            has its outward normal on the outer side at an extreme point, so closed pieces come out pointing outwards.
 *   comp_out [B,M] int, nullable: the smallest point index, inside the cloud, of the point's connected component.
 * The output is bit-determined by the inputs, does not depend on the input signs (apart from dots that are exactly 0) and is
 * the same from run to run.  Limits: a neighbour graph can fall into several components even on one surface; each is oriented
 * on its own by the extreme-point rule, which is right for closed pieces and a guess for fragments (components are not joined);
 * sheets closer together than a neighbourhood can still flip.
 * Boruvka rounds with a flip bit per vertex; ceil(log2 M) rounds (M: the largest cloud) are enqueued without a host read
 * between launches, finished rounds return at once; every loop in every kernel has a constant or host-given bound; integer atomics only.
 * ws: pf_normals_orient_ws_bytes(m, B) bytes of device memory, 16-byte aligned (37 bytes per point), rebuilt by every call.
 * normal_out may alias normal_in.  2 <= K <= PF_KNN_GRID_MAX_K, else PF_ERR_UNSUPPORTED.  Before any device work: PF_ERR_NULL
 * (ws too; viewpoint and comp_out may be null), PF_ERR_SHAPE (B, M or m[i] <= 0, K > M or K > any m[i], more than 2^31 / 3
 * points, misaligned ws), PF_ERR_UNSUPPORTED, PF_ERR_WORKSPACE (ws_bytes too small). */
/* bytes of workspace for B clouds of m[i] points (pf_normals_orient: m[i] = M for all); negative PF_ERR_* on a bad argument */
long long pf_normals_orient_ws_bytes(const int* m, int B);
int pf_normals_orient(const float* pts, const float* normal_in, const int* idx, int B, int M, int K, const float* viewpoint,
                      void* ws, long long ws_bytes, float* normal_out, int* comp_out, void* stream);
/* pf_normals_orient per cloud of a ragged pass: pts, normal_in [sum m, 3], idx [sum m, K] (pf_knn_large_ragged, indices inside
 * the cloud), m: HOST array of B ints.  Edges never cross clouds: one forest over the packed tensor.  Every cloud gets, bit for
 * bit, what pf_normals_orient gives it alone. */
int pf_normals_orient_ragged(const float* pts, const float* normal_in, const int* idx, const int* m, int B, int K,
                             const float* viewpoint, void* ws, long long ws_bytes, float* normal_out, int* comp_out, void* stream);

/* ---- surface from an oriented cloud: IMLS and marching tetrahedra (csrc/recon.hip) ---------------------------
 * Three stages on the device: mark a narrow band of grid corners around the points, compute an implicit value at those corners
 * from the K nearest oriented points, extract the zero set with marching tetrahedra, vertices welded by grid-edge id.
 *   Grid      (host) cell size h; with pad = 3, in double, o_a = lo_a - pad h and D_a = ceil((hi_a - lo_a) / h) + 2 pad + 1
 *             corners per axis, lo / hi the fp32 box of the points.  Corner coordinates are three fp32 tables made on the host,
 *             g_a[i] = float32(o_a + i h), double rounded once; the kernels read the tables and never recompute a coordinate, so
 *             no contraction choice can move a corner.  x is the fastest index: corner c = (k D_y + j) D_x + i.  Every D_a >= 2
 *             (else PF_ERR_SHAPE) and D_x D_y D_z <= PF_RECON_MAX_CORNERS (else PF_ERR_UNSUPPORTED): dense arrays over the box,
 *             the band only limits where work is done.
 *   Cell      cell_a(p) = (number of entries of g_a that are <= p_a) - 1, clamped to 0 .. D_a - 2: a binary search in the table
 *             itself, monotone and exact by construction.
 *   Band      pf_recon_mark: flags [D_z, D_y, D_x] bytes, cleared, then every point stores 1 at the 4 x 4 x 4 corners
 *             cell_a - 1 .. cell_a + 2 of its cell (those inside the box; pad = 3 keeps all of them inside).  Plain stores of one
 *             value, no atomics.  A cell is ACTIVE when all 8 of its corners are flagged.
 *   Value     pf_imls: query [Q,3], pts / normals [N,3] (unit normals), idx [Q,K] from pf_knn_grid(ref = pts, query), entries
 *             clamped to the cloud.  Per query x, in double: d2_k = |x - p_k|^2 from the coordinates (not the search's fp32
 *             value), w_k = exp(-(d2_k - d2_0) / sigma_h^2) - neighbour 0 has weight 1, the denominator cannot underflow -
 *             f(x) = sum_k w_k (n_k . (x - p_k)) / sum_k w_k, summed for k = 0 .. K - 1 in that order, rounded to fp32 once.
 *             sigma_h = sigma h > 0 and 1 / sigma_h^2 finite.  One lane per query.
 *   Tets      INSIDE means f < 0.  Every active cell with lower corner c is cut into 6 tets along its main diagonal: for the
 *             permutations pi of (x, y, z) in lexicographic order, v0 = c, v1 = v0 + e_pi0, v2 = v1 + e_pi1, v3 = c + (1,1,1).
 *             The cut is the same in every cell, so tet faces match across cells.
 *   Edges     7 classes by offset: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1) = 0 .. 6.  An edge is owned by its
 *             lower corner: edge id = 7 c + class, as long long.
 *   Triangles per tet: 1 or 3 corners inside - one triangle on the three edges at the lone corner, the others in tet order;
 *             2 inside - with the inside pair a < b and the outside pair c < d in tet order, (ac, ad, bd) and (ac, bd, bc).
 *             The last two edges are swapped where needed so that the triangle's normal points to the positive side
 *             (counter-clockwise seen from outside), decided in integers as if every vertex sat at its edge's midpoint, from a
 *             table generated in code: a triangle that an exact 0 in f makes degenerate is oriented like its neighbours.
 *   Order     triangles go out in the order (cell index c, tet 0 .. 5, triangle 0 .. 1).  pf_mtet_count: count [D_z, D_y, D_x]
 *             ints, the triangles of cell c (0 where c is no active cell).  pf_mtet_emit: first [D_z, D_y, D_x] long long, the
 *             exclusive prefix sum of count; T its total; edge_ids [T,3] long long.  Triangles outside 0 .. T - 1 are dropped.
 *   Vertices  pf_mtet_vertices: edge_ids [V] (the distinct ids, ascending) -> verts [V,3].  Vertex (a, b), a < b by corner index,
 *             sits at t = f_a / (f_a - f_b), an IEEE fp32 division; per component v = g[a] + t (g[b] - g[a]) with the subtraction,
 *             the product and the sum as three separately rounded fp32 operations.  An id that names no edge of the box: (0,0,0).
 * The mesh is bit-determined by the inputs and the same from run to run.  f is read at flagged corners only.
 * Every loop in every kernel has a constant or host-given bound; no spin-wait, no grid barrier, no cooperative launch, no
 * atomics.  Before any device work: PF_ERR_NULL; PF_ERR_SHAPE (N, Q, T or V <= 0, a D_a < 2, K > N, more than 2^31 / 3 points or
 * queries, sigma_h not positive, T > 12 or V > 7 times the corners); PF_ERR_UNSUPPORTED (K outside 1 .. PF_KNN_GRID_MAX_K, a
 * box over the cap). */
#define PF_RECON_MAX_CORNERS (1 << 26)
int pf_recon_mark(const float* pts, int N, const float* gx, const float* gy, const float* gz, int Dx, int Dy, int Dz,
                  unsigned char* flags, void* stream);
int pf_imls(const float* query, const float* pts, const float* normals, const int* idx, int Q, int N, int K, double sigma_h,
            float* f, void* stream);
/* the generated triangle table as the kernels hold it, copied to HOST memory (no device work): corner[6][4], the cube corner
 * x | y << 1 | z << 2 of every tet vertex; ntri[6][16], triangles per tet and sign pattern (bit v: vertex v inside);
 * edge[6][16][2][3], per triangle its three edges as (owner's cube corner) << 3 | class.  Returns PF_MTET_TABLE_BYTES. */
#define PF_MTET_TABLE_BYTES 696
int pf_mtet_table(unsigned char* out, int bytes);
int pf_mtet_count(const float* f, const unsigned char* flags, int Dx, int Dy, int Dz, int* count, void* stream);
int pf_mtet_emit(const float* f, const unsigned char* flags, int Dx, int Dy, int Dz, const long long* first, long long T,
                 long long* edge_ids, void* stream);
int pf_mtet_vertices(const long long* edge_ids, long long V, const float* f, const float* gx, const float* gy, const float* gz,
                     int Dx, int Dy, int Dz, float* verts, void* stream);

/* ---- closing holes: the band grows at its exits (csrc/recon.hip; DESIGN.md 8e "Closing holes") ------------------------------
 * Where the samples leave a gap wider than the band, the zero set of f runs out of the active cells and the mesh ends there.
 * f is defined everywhere (pf_imls takes the K nearest points wherever the query lies), so the host extends the band exactly
 * where the surface leaves it, for up to R <= PF_RECON_GROW_MAX_ROUNDS rounds (a host-given bound), one pf_recon_grow per round,
 * in the dense layout only.  Band, value and extraction are the entry points above, unchanged.
 *   Grid      (host) pad = 3 + R corners per side: D_a = ceil((hi_a - lo_a) / h) + 7 + 2 R, and the tables are the old ones
 *             shifted, g_a[i] = float32(o_a + (i - R) h) with the unchanged o_a = lo_a - 3 h, in double.  R = 0 is the expression
 *             above.  The shift is monotone in the corner index, so edge ids keep their order and, on a cloud where nothing
 *             grows, the mesh is the R = 0 mesh bit for bit.  PF_RECON_MAX_CORNERS applies to the padded box.
 *   Exit      an inactive cell c (not on the last index of any axis) with one of its six face neighbours inside the grid, for
 *             which both hold: the neighbour is ACTIVE (all 8 of its corners flagged), and the shared face's four corners do
 *             not all agree in f < 0.  Those four corners belong to the active neighbour, so they are flagged and their f is
 *             valid.  -0.0 and +0.0 are both "not inside", as in the extraction.
 *   Round     pf_recon_grow: added [D_z, D_y, D_x] bytes, cleared, then every exit stores 1 at its own 8 corners.  Plain stores
 *             of one value, no atomics; reads go to flags and f only, so nothing depends on the order of lanes.  The host takes
 *             new = added & ~flags, compacts it in ascending corner index, evaluates pf_knn_grid and pf_imls at the new corners
 *             only, scatters the values into f and sets flags |= added.
 *   Stop      after R rounds, or earlier when a round finds no exit (an exit is inactive, so one of its corners is new: no new
 *             corner, no exit).  The mesh is extracted once, after the last round.
 * Marching tetrahedra cut every cell the same way, so a mesh edge used by one triangle lies on a face between an active and an
 * inactive cell that the zero set crosses - an exit's face: "no exit left" and "no open edge" coincide, up to exact zeros of f.
 * A hole shrinks from all sides by at most a cell per round.  A real boundary grows outward by at most R cells along the tangent
 * planes and stays a boundary.  One lane per cell, every index checked, constant loop bounds, no atomics, no spin-wait, no grid
 * barrier, no cooperative launch.  Before any device work: PF_ERR_NULL; PF_ERR_SHAPE (a D_a < 2); PF_ERR_UNSUPPORTED (a box over
 * the cap). */
#define PF_RECON_GROW_MAX_ROUNDS 64
int pf_recon_grow(const float* f, const unsigned char* flags, int Dx, int Dy, int Dz, unsigned char* added, void* stream);

/* ---- the same surface in a block-sparse layout (csrc/recon_sparse.hip; DESIGN.md 8e "Block-sparse band") -------------------
 * A second layout of the stages above whose memory and work follow the band, not the box.  It returns the dense layout's mesh
 * bit for bit (vertices, faces and their order) wherever that one runs, and the same contract's mesh beyond its cap.
 *   Grid      virtual: the host rule, the tables and the cell rule are the dense ones; corner c = (k D_y + j) D_x + i is a long
 *             long and no array has D_x D_y D_z entries.  Every D_a >= 2 (else PF_ERR_SHAPE) and D_a <= PF_RECON_SPARSE_MAX_AXIS
 *             = 2^20 (else PF_ERR_UNSUPPORTED): 7 c + 6 < 2^63, a table is at most 4 MB.
 *   Blocks    PF_RECON_BLOCK = 8 corners per axis.  Corner (i, j, k) lies in block (i >> 3, j >> 3, k >> 3) at slot
 *             (k & 7) << 6 | (j & 7) << 3 | (i & 7).  Block key = (bk NB_y + bj) NB_x + bi as long long, NB_a = ceil(D_a / 8).
 *             A block array is [NB, 512]; slot number = 512 b + slot, b the block's position in the list.
 *   List      pf_recon_block_keys: keys [N, 8] long long, per point the blocks that its 4 x 4 x 4 corners (clipped to the grid as
 *             in pf_recon_mark) touch: entry o = ox | oy << 1 | oz << 2 is the block of the FIRST (o_a = 0) or LAST (o_a = 1) of
 *             its corners along each axis - four corners span at most two blocks, and the same key comes twice where one block
 *             holds all four.  The host's ascending list of the distinct keys, blocks [NB], IS the layout: 1 <= NB <=
 *             PF_RECON_SPARSE_MAX_BLOCKS = 2^21 (else PF_ERR_UNSUPPORTED), so a slot number fits an int, and NB <= NB_x NB_y NB_z
 *             (else PF_ERR_SHAPE).  A block is found by a binary search in the list, 32 halvings; there is no hash table.
 *   Links     pf_recon_block_links: links [NB, 8] ints, entry o the list position of the block at offset (o & 1, o >> 1 & 1,
 *             o >> 2 & 1), -1 where the list (or the grid) has none; entry 0 is the block itself.  A cell's corners and an
 *             edge's upper corner are at +0 / +1, so the links are all that cells and edges need.
 *   Band      pf_recon_mark_sparse: flags [NB, 512] bytes, cleared, then every point stores 1 at its 4 x 4 x 4 corners, after
 *             finding its at most 8 blocks once.  Slots beyond D_a in a last block are never flagged.  A corner whose block is
 *             not listed is skipped (the list of pf_recon_block_keys misses none).
 *   Value     pf_knn_grid and pf_imls as above on the flagged slots in ascending slot number, scattered into f [NB, 512]; one
 *             lane per query, so the order of the queries changes no bit.
 *   Count     pf_mtet_count_sparse: count [NB, 512] ints, per slot the triangles of the cell whose lower corner it is, by the
 *             dense rules; the cell's 8 corners are reached through the links, and it is active when all are flagged.
 *   Order     triangles go out in ascending GLOBAL cell index c, then tet, then triangle: the dense order.  The host lists the
 *             slot numbers with a non-zero count sorted by their c (distinct keys) - cells [M] long long - with first [M] long
 *             long, the exclusive prefix sum of their counts in that order, T its total.  pf_mtet_emit_sparse: edge_ids [T,3],
 *             7 (owner's global c) + class.  Entries of cells outside 0 .. 512 NB - 1, cells that are not active, and triangles
 *             outside 0 .. T - 1 are dropped.
 *   Vertices  pf_mtet_vertices_sparse: id -> (i, j, k) by 64-bit division -> the block by a search -> f_a; the upper corner
 *             through the block's link -> f_b; then the dense arithmetic.  An id that names no edge of the grid, or whose
 *             corners lie in no listed block: (0,0,0).
 * Every index that comes from a list (keys, links, slots, first, ids) is clamped or checked; every loop has a constant or
 * host-given bound; no atomics, no grid barrier, no cooperative launch.  Before any device work: PF_ERR_NULL; PF_ERR_SHAPE
 * (N, NB, M, T or V <= 0, a D_a < 2, more than 2^31 / 3 points, NB over the grid's blocks, M > 512 NB, T > 12 M, V > 7 x 512
 * NB); PF_ERR_UNSUPPORTED (an axis or a block list over its cap). */
#define PF_RECON_BLOCK 8
#define PF_RECON_SPARSE_MAX_AXIS (1 << 20)
#define PF_RECON_SPARSE_MAX_BLOCKS (1 << 21)
int pf_recon_block_keys(const float* pts, int N, const float* gx, const float* gy, const float* gz, int Dx, int Dy, int Dz,
                        long long* keys, void* stream);
int pf_recon_block_links(const long long* blocks, int NB, int Dx, int Dy, int Dz, int* links, void* stream);
int pf_recon_mark_sparse(const float* pts, int N, const float* gx, const float* gy, const float* gz, int Dx, int Dy, int Dz,
                         const long long* blocks, int NB, unsigned char* flags, void* stream);
int pf_mtet_count_sparse(const float* f, const unsigned char* flags, const long long* blocks, const int* links, int NB, int Dx,
                         int Dy, int Dz, int* count, void* stream);
int pf_mtet_emit_sparse(const float* f, const unsigned char* flags, const long long* blocks, const int* links, int NB, int Dx,
                        int Dy, int Dz, const long long* cells, const long long* first, long long M, long long T,
                        long long* edge_ids, void* stream);
int pf_mtet_vertices_sparse(const long long* edge_ids, long long V, const float* f, const long long* blocks, const int* links,
                            int NB, const float* gx, const float* gy, const float* gz, int Dx, int Dy, int Dz, float* verts,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PUFLOW_HIP_H */
