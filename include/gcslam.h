/*
 * gcslam.h — C-ABI of libgcslam: the MI355X-native GC-SLAM v2 per-scan hot path.
 *
 * Drop-in boundary for the reference's operator API (fl_slam_poc.backend.operators,
 * docs/OPERATOR_CONTRACTS.md:3,35-38): every operator of the 14-step per-scan pipeline is an
 * `extern "C"` entry over plain pointers and sizes. The Python host package (gcslam) binds it
 * with ctypes and rebuilds the reference's (Result, CertBundle, ExpectedEffect) tuples.
 *
 * Conventions
 *  - All arithmetic is IEEE f64, as in the reference (jax_enable_x64, common/jax_init.py:32).
 *  - Array arguments named d_* are DEVICE pointers (gc_buffer_alloc), row-major, C-contiguous.
 *    Batched entries take H hypotheses stacked on the leading axis. Host pointers are h_*.
 *  - Every entry is enqueued on the context's HIP stream and returns immediately unless noted;
 *    gc_ctx_synchronize() waits. Entries never retain caller pointers.
 *  - Return codes: GC_OK, GC_ERR_ARG (shape/argument error -> Python ValueError),
 *    GC_ERR_RUNTIME (HIP/RCCL failure -> RuntimeError). gc_last_error() has the message.
 *  - Re-entrant: no global mutable state; one gc_ctx (stream) per calling thread
 *    (backend_node.py:1340-1381 worker-thread model).
 */
#ifndef GCSLAM_H_
#define GCSLAM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GC_OK 0
#define GC_ERR_ARG 1
#define GC_ERR_RUNTIME 2

/* Per-bin statistics record written by the bin kernels (doubles per bin):
 * [0] N  [1:4] s_dir  [4:13] S_dir_scatter  [13:16] p_bar  [16:25] Sigma_p  [25] kappa
 * [26:29] sum_p  [29:38] sum_ppT   (ScanBinStats, archive/legacy_operators/binning.py:39-48) */
#define GC_BIN_STATS 38
/* Per-hypothesis bin certificate row (doubles):
 * [0] ess [1] support_frac [2] psd_projection_delta_total [3] max_mass_epsilon_ratio
 * [4] avg_entropy (soft-assign) [5] max_resp [6] sum of deskewed weights [7] trigger magnitude */
#define GC_BIN_CERT 8

typedef struct gc_ctx gc_ctx;
typedef struct gc_event gc_event;

/* ------------------------------------------------------------------ runtime */
int32_t gc_version(void);
/* Message of the last failing call on this ctx (ctx may be NULL for creation errors). */
const char* gc_last_error(const gc_ctx* ctx);
int32_t gc_device_count(int32_t* count);
int32_t gc_ctx_create(int32_t device, gc_ctx** out);
int32_t gc_ctx_destroy(gc_ctx* ctx);
/* Waits for everything enqueued on the ctx stream. Like every host wait in libgcslam it is bounded
 * (fail fast, backend_node.py:2205-2210 log and re-raise): after the context's wait timeout it returns
 * GC_ERR_RUNTIME, and an RCCL communicator initialised on this context is aborted first, so a rank whose
 * peer died does not stay in an all-gather. Its asynchronous error is polled during the wait. */
int32_t gc_ctx_synchronize(gc_ctx* ctx);
/* The bound of every host wait on this context, seconds (default: $GC_WAIT_TIMEOUT_S, else 300). */
int32_t gc_ctx_set_wait_timeout(gc_ctx* ctx, double seconds);
/* Test entries of the bounded wait. gc_test_bounded_wait runs the wait loop on a condition that
 * completes after ready_after_polls polls (< 0: never) with no device involved: GC_OK, or
 * GC_ERR_RUNTIME once timeout_s has passed; h_waited_ms receives the time spent. gc_test_device_spin
 * enqueues a one-thread kernel that keeps the stream busy for `seconds` (<= 10) and then exits. */
int32_t gc_test_bounded_wait(double timeout_s, int64_t ready_after_polls, double* h_waited_ms);
int32_t gc_test_device_spin(gc_ctx* ctx, double seconds);
/* Test entry of the library's device radix sort (the PrimitiveMap cull / insert / merge and the map view's
 * per-tile order): d_keys_in (n_seg x L doubles, n_seg * L < 2^32) sorted within each segment of L keys,
 * ascending (or descending), stable (equal keys, -0.0 and +0.0 included, in input order), into
 * d_keys_out, with d_vals_in (32-bit; NULL: keys only) permuted alike into d_vals_out. */
int32_t gc_test_radix_sort(gc_ctx* ctx, const double* d_keys_in, const uint32_t* d_vals_in, int64_t n_seg, int64_t L,
                           int32_t descending, double* d_keys_out, uint32_t* d_vals_out);
/* Device buffers from the context's arena (SURVEY §8b ownership): gc_buffer_free returns a block to a
 * per-size-class cache and the next allocation of that class takes it back, so a steady-state chain of
 * per-operator calls performs no hipMalloc / hipFree and no synchronisation. All work on arena buffers
 * must be ordered on the context's stream (as every libgcslam entry is). gc_ctx_trim returns the cached
 * blocks to HIP; gc_ctx_alloc_stats: [hipMalloc calls, hipFree calls, arena reuses, live buffers,
 * live bytes, cached bytes]. */
int32_t gc_buffer_alloc(gc_ctx* ctx, uint64_t bytes, void** d_ptr);
int32_t gc_buffer_free(gc_ctx* ctx, void* d_ptr);
int32_t gc_ctx_trim(gc_ctx* ctx);
int32_t gc_ctx_alloc_stats(gc_ctx* ctx, int64_t* h_out6);
/* Copies on the context's stream. An upload returns once the caller's buffer may be reused: up to
 * 512 KiB it is copied into the context's pinned staging ring and the DMA is left in flight (later work
 * on the stream is ordered after it), larger ones are waited for. A download is waited for.
 * When a staged upload returns, the destination does NOT hold the data yet: only work on the context's
 * stream is ordered after the copy. A consumer on another stream (or another process reading the buffer)
 * must gc_ctx_sync first, or wait on an event recorded on the context's stream after the upload
 * (gc_event_record). */
int32_t gc_buffer_upload(gc_ctx* ctx, void* d_dst, const void* h_src, uint64_t bytes);
int32_t gc_buffer_download(gc_ctx* ctx, void* h_dst, const void* d_src, uint64_t bytes);
int32_t gc_buffer_copy(gc_ctx* ctx, void* d_dst, const void* d_src, uint64_t bytes);
int32_t gc_buffer_memset(gc_ctx* ctx, void* d_dst, int32_t value, uint64_t bytes);
/* HIP events on the ctx stream (for in-process kernel timing). */
int32_t gc_event_create(gc_ctx* ctx, gc_event** out);
int32_t gc_event_destroy(gc_event* ev);
int32_t gc_event_record(gc_ctx* ctx, gc_event* ev);
int32_t gc_event_elapsed_ms(gc_event* start, gc_event* stop, float* ms);

/* ------------------------------------------------------------------ a1 PointBudgetResample
 * Replaces backend/operators/point_budget.py:50-109 (_point_budget_resample_core) and the
 * stride of :160. stride = max(1, ceil(n_in / n_cap)); selection = arange(0, n_in, stride).
 * Outputs (n_cap rows, zero padded): d_points_out (n_cap,3), d_t_out, d_w_out (n_cap),
 * d_ring_out/d_tag_out (n_cap, u8; inputs may be NULL -> zeros), d_idx_out (n_cap, int64,
 * -1 padded). d_scalars_out (8): [mass_in, mass_selected, mass_scale, ess, sum_w_out,
 * n_selected, stride, support_frac]. */
int32_t gc_point_budget_resample(gc_ctx* ctx, const double* d_points, const double* d_t,
                                 const double* d_w, const uint8_t* d_ring, const uint8_t* d_tag,
                                 int64_t n_in, int64_t n_cap, double* d_points_out, double* d_t_out,
                                 double* d_w_out, uint8_t* d_ring_out, uint8_t* d_tag_out,
                                 int64_t* d_idx_out, double* d_scalars_out);

/* ------------------------------------------------------------- PointCloud2
 * parse_pointcloud2_vlp16 (backend/backend_node.py:377-468) + the no-TF base transform
 * p_base = R p + t (backend_node.py:1677-1690) on the device. d_data: the message's raw bytes
 * (n_points * point_step, little-endian). h_fields (10 int32): [x_off, x_type, y_off, y_type,
 * z_off, z_type, ring_off, ring_type, time_off, time_type] with sensor_msgs/PointField datatype
 * codes (1 INT8 .. 8 FLOAT64); time_off = -1 when the cloud has no t/time field (every point gets
 * header_stamp). Times are divided by 1e9 when any raw time exceeds 1e6 (ns-stamped drivers).
 * Non-finite coordinates become ±1e6 (GC_NONFINITE_SENTINEL); weights are the range sigmoid of
 * the sensor-frame distance; ring is the field cast to uint8; tag = 0. */
int32_t gc_pointcloud2_parse(gc_ctx* ctx, const uint8_t* d_data, int64_t n_points, int32_t point_step,
                             const int32_t* h_fields, double header_stamp, const double* h_R9, const double* h_t3,
                             double* d_points_out, double* d_t_out, double* d_w_out, uint8_t* d_ring_out,
                             uint8_t* d_tag_out);

/* ------------------------------------------------------------------ a4 DeskewConstantTwist
 * Replaces backend/operators/deskew_constant_twist.py:31-69 for H twists over one point set:
 * p0 = Exp(α ξ_h)^{-1} p, α = (t - t0)/max(t1 - t0, 1e-12); w_out = w · window(t).
 * d_xi (H,6); d_points_out (H,n,3); d_w_out (H,n); d_sum_w_out (H) = Σ w_out (retained cert). */
int32_t gc_deskew_constant_twist(gc_ctx* ctx, int32_t H, int64_t n, const double* d_points,
                                 const double* d_t, const double* d_w, double t0, double t1,
                                 const double* d_xi, double* d_points_out, double* d_w_out,
                                 double* d_sum_w_out);

/* Ray directions (pipeline.py:589-593): d = (p - o) / (||p - o|| + eps_mass). (rows = H*n) */
int32_t gc_point_directions(gc_ctx* ctx, int64_t rows, const double* d_points, const double* h_origin3,
                            double eps_mass, double* d_dirs_out);

/* ------------------------------------------------------------------ a5 BinSoftAssign
 * Replaces archive/legacy_operators/binning.py:56-76 (_bin_soft_assign_core), batched over H.
 * d_dirs (H,n,3), any norm; d_bins (B,3), B <= 64; tau > 0;
 * d_resp_out (H,n,B) = softmax(dirs·binsᵀ/τ) shifted by the row maximum as jax.nn.softmax;
 * d_bin_index_out (H,n) int32 = argmax_b of the un-fused f64 d0*b0+d1*b1+d2*b2 (lowest index
 * on ties; may be NULL); d_cert_out (H,2) = [avg_entropy, max_resp]. */
int32_t gc_bin_soft_assign(gc_ctx* ctx, int32_t H, int64_t n, int32_t B, const double* d_dirs,
                           const double* d_bins, double tau, double* d_resp_out,
                           int32_t* d_bin_index_out, double* d_cert_out);

/* ------------------------------------------------------------------ a6 ScanBinMomentMatch
 * Replaces binning.py:139-209 (_scan_bin_moment_match_core) incl. KappaFromResultant
 * (kappa.py:130-169) and InvMass (primitives.py:195-212), batched over H.
 * d_points (H,n,3), d_covs (H,n,3,3) or NULL (= zeros), d_w (H,n), d_resp (H,n,B),
 * d_lambda (H,n) or NULL (= ones), h_origin3 (host, 3). Outputs d_stats_out (H,B,GC_BIN_STATS)
 * and d_cert_out (H,GC_BIN_CERT) (entries [4:7] zero). */
int32_t gc_scan_bin_moment_match(gc_ctx* ctx, int32_t H, int64_t n, int32_t B, const double* d_points,
                                 const double* d_covs, const double* d_w, const double* d_resp,
                                 const double* d_lambda, const double* h_origin3, double eps_psd,
                                 double eps_mass, double* d_stats_out, double* d_cert_out);

/* Fused a1->a4->a5->a6 over H hypotheses of one raw scan (the batched pipeline's hot kernel):
 * budget selection (stride from n_in/n_cap, weights x d_budget_scalars[2]), per-hypothesis
 * deskew by d_xi (H,6), directions from h_origin3, soft assignment to d_bins (B,3) at tau and
 * moment accumulation — responsibilities never touch HBM. Same outputs as the contract pair
 * (d_stats_out (H,B,GC_BIN_STATS), d_cert_out (H,GC_BIN_CERT) incl. [4:7]).
 * d_budget_scalars: the 8 scalars written by gc_point_budget_resample / gc_budget_stats.
 * tau >= GC_FUSED_TAU_MIN (the table exp's range; the contract gc_bin_soft_assign takes any tau).
 * iters: 256-point iterations per workgroup (launch geometry; it changes only the summation
 * order): 0 = chosen from the grid size (16 at 64k points x 256 hypotheses, 1 below ~1024
 * workgroups), 1..64 = forced. */
#define GC_FUSED_TAU_MIN 3e-3
int32_t gc_scan_bins_fused(gc_ctx* ctx, int32_t H, int64_t n_in, int64_t n_cap, int32_t B,
                           const double* d_points_raw, const double* d_t_raw, const double* d_w_raw,
                           const double* d_budget_scalars, double t0, double t1, const double* d_xi,
                           const double* d_bins, double tau, const double* h_origin3,
                           double eps_psd, double eps_mass, double* d_stats_out, double* d_cert_out,
                           int32_t iters);

/* The task plan of the batched pipeline's bins launch (host-only: no context, no device): how the
 * ceil(n_cap / 256) 256-point units of a budgeted scan are cut into chunks for a shard whose chunk
 * geometry is sized for H_geom hypotheses (gc_pipeline geom_H, or the shard's own count) on a device
 * of cu_count compute units. Chunks [0, k1) hold iters x 256 points, the next k2 iters_short x 256,
 * the rest iters_tiny x 256; a hypothesis's records are summed in chunk order, so the plan fixes the
 * order of summation.
 * out8 = [iters, iters_short, iters_tiny, k1, k2, chunks, ahead (0/1), pullers]; ahead: the
 * look-ahead form of the bins kernel runs (short tasks), otherwise the late-ticket form; pullers:
 * the resident bin workgroups, 2 x cu_count.
 * GC_ERR_ARG for H_geom < 1, n_cap < 1, cu_count < 1 or a NULL out8. */
int32_t gc_bins_task_plan(int32_t H_geom, int64_t n_cap, int32_t cu_count, int64_t* out8);

/* Budget reduction only (no gather): writes the 8 budget scalars. */
int32_t gc_budget_stats(gc_ctx* ctx, const double* d_w, int64_t n_in, int64_t n_cap,
                        double* d_scalars_out);

/* kappa_from_resultant_batch (kappa.py:130-169). */
int32_t gc_kappa_from_resultant_batch(gc_ctx* ctx, int64_t n, const double* d_R, double eps_r,
                                      double d, double r0, double tau, double* d_kappa_out);

/* domain_projection_psd_core (primitives.py:80-123) over `batch` d x d matrices, any 1 <= d <= 512
 * (cyclic Jacobi; an odd d is padded with a decoupled zero row/column that the certificate
 * ignores). d_cert_out (batch,6) = [projection_delta, sym_delta, eig_min, eig_max, cond, nnc]. */
int32_t gc_domain_projection_psd_batch(gc_ctx* ctx, int32_t batch, int32_t d, const double* d_M,
                                       double eps_psd, double* d_M_out, double* d_cert_out);

/* ------------------------------------------------------------------ batched scan pipeline
 * Replaces the per-hypothesis loop + combine + IW apply of backend_node.py:2036-2119 (and
 * process_scan_single_hypothesis, pipeline.py:316-1591, with the legacy bin path a4-a8 of
 * SURVEY §3.2) by one device-resident driver over this rank's shard of hypotheses. */
typedef struct gc_pipeline gc_pipeline;
typedef struct gc_comm gc_comm;

typedef struct {
  int32_t H_total;   /* hypotheses per scan (all ranks) */
  int32_t h_begin;   /* first global hypothesis of this rank */
  int32_t h_count;   /* hypotheses on this rank (<= 1024) */
  int32_t B;         /* bins (<= 64) */
  int32_t M;         /* IMU slots (GC_MAX_IMU_PREINT_LEN = 512) */
  int32_t world_size;
  int32_t rank;
  int32_t geom_hyps; /* 0: the bins launch's chunk geometry follows h_count (and the CU count);
                        k > 0: as for a shard of k hypotheses, so shards of different sizes sum each
                        hypothesis's points in the same order (cross-world-size bit-reproducibility
                        of the per-hypothesis results) */
  int64_t n_in_max;  /* raw points per scan (max) */
  int64_t n_cap;     /* N_POINTS_CAP */
} gc_pipeline_dims;

/* The pipeline's configuration (PipelineConfig, pipeline.py:96-160; constants.py). Like every gc_*_cfg
 * below it holds doubles only, so it has no padding and a caller may fill it as a double array in member
 * order. */
typedef struct {
  double tau;
  double origin_x; /* the lidar origin in the base frame */
  double origin_y;
  double origin_z;
  double eps_psd;
  double eps_lift;
  double eps_mass;
  double lambda_ou;
  double c_frob;
  double forgetting_factor;
  double weight_floor;
  double power_beta_min;
  double power_beta_exc_c;
  double power_beta_z_c;
  double alpha_min;
  double alpha_max;
  double c0_cond;
  double nu_max;
  double planar_z_ref;      /* GC_PLANAR_Z_REF (constants.py:294) */
  double planar_z_sigma;    /* GC_PLANAR_Z_SIGMA (constants.py:305) */
  double planar_vz_sigma;   /* GC_PLANAR_VZ_SIGMA (constants.py:310) */
  double imu_gravity_scale; /* PipelineConfig.imu_gravity_scale (pipeline.py:141) */
} gc_pipeline_cfg;

#define GC_PIPE_MAX_SLOTS 8
/* map bin record (B x 26): [S_dir 3, S_dir_scatter 9, N_dir, N_pos, sum_p 3, sum_ppT 9] */
#define GC_MAP_REC 26
/* map-derived record (B x 17): [mu_dir 3, kappa, centroid 3, Sigma_c 9, pad] */
#define GC_MAP_DER 17
/* IMU/odom-branch cert row (10): ess odom/imu/gyro, support odom/imu/gyro, exc_dt, exc_ex,
 * nll_per_ess sum, trigger-magnitude sum */
#define GC_IO_CERT 10
/* per-hypothesis diagnostics (40): [0:6] world pose of the final belief, 6 T, 7 beta, 8 alpha,
 * 9 s_dt, 10 s_ex, 11 anchor rho, 12 frobenius strength, 13 cond_pose6, 14 ess_total,
 * 15 dt_asymmetry, 16 z_to_xy, 17 nll_per_ess, 18 MF trigger, 19 planar trigger,
 * 20 fusion psd delta, [21:24] t_wls, [24:27] log R_mf, [27:30] MF singular values,
 * [30:36] xi_body, 36 support_frac, 37 excitation_total, 38 |mu_final|^2 (barycenter spread),
 * 39 eigmin_pose6 (clipped at eps_psd, pipeline.py:1157-1168) */
#define GC_HYP_DIAG 40
/* combined output (GC_COMB_LEN): L 484, h 22, z_lin 22, X_anchor(hyp 0) 6, then
 * [stamp, psd_delta, eig_min, eig_max, cond, nnc, ess, support_frac, mass_eps_ratio,
 *  floor_adjustment, spread_proxy, 5 pad]. The conditioning fields are always filled: when the
 *  scan path certified the barycenter PSD by Cholesky, gc_pipeline_get_combined computes them from
 *  the stored combined L on demand (one extra launch, off the scan path). */
#define GC_COMB_LEN (484 + 22 + 22 + 6 + 16)

int32_t gc_pipeline_create(gc_ctx* ctx, const gc_pipeline_dims* dims, const gc_pipeline_cfg* cfg, gc_pipeline** out);
int32_t gc_pipeline_destroy(gc_pipeline* p);
int32_t gc_pipeline_set_bins(gc_pipeline* p, const double* h_bins);
int32_t gc_pipeline_set_beliefs(gc_pipeline* p, const double* h_X, const double* h_z, const double* h_L,
                                const double* h_h, const double* h_stamp);
int32_t gc_pipeline_get_beliefs(gc_pipeline* p, double* h_X, double* h_z, double* h_L, double* h_h,
                                double* h_stamp);
int32_t gc_pipeline_set_weights(gc_pipeline* p, const double* h_weights);
int32_t gc_pipeline_set_io_evidence(gc_pipeline* p, const double* h_L, const double* h_h, const double* h_cert);
/* IMU/odom branch source: GC_IO_GIVEN uses the evidence of gc_pipeline_set_io_evidence (synthetic
 * input; calling it selects this mode); GC_IO_COMPUTED (default) evaluates _compute_imu_odom_branch (pipeline.py:595-776) on the
 * device each scan from the slot's odometry (gc_pipeline_stage_odom) and IMU window. */
#define GC_IO_GIVEN 0
#define GC_IO_COMPUTED 1
int32_t gc_pipeline_set_io_mode(gc_pipeline* p, int32_t mode);
/* Odometry of a scan slot (backend_node.py:1748-1765): relative pose [t, rotvec] (6), pose
 * covariance (6,6) in [trans, rot] order, body twist [v, ω] (6), twist covariance (6,6). */
int32_t gc_pipeline_stage_odom(gc_pipeline* p, int32_t slot, const double* h_pose6, const double* h_cov36,
                               const double* h_twist6, const double* h_twist_cov36);
/* Per-hypothesis IMU/odom-branch internals of the last scan (GC_IO_COMPUTED), (Hl, GC_IO_PARTS):
 * [0:6] odom se3 residual, 6 kappa, 7 ess_weighted, 8 ess_raw, 9 mean_reliability,
 * 10 transport_sigma, 11 Rbar, 12 imu dependence scale, [13:16] gyro r_rot, [16:19] preint r_vel,
 * [19:22] preint r_pos, 22 planar r_z, 23 v_z, [24:27] odom-velocity r_vel, 27 yaw-rate r_wz,
 * [28:31] kinematic r_trans, [31:34] kinematic r_rot, 34 odom dependence scale, 35 odom nll,
 * 36 imu nll, 37 gyro nll, 38 dt_int, 39 trigger-magnitude sum of the 11 certs.
 * gc_pipeline_get_io_evidence reads back (L_io, h_io, cert row) of the last scan. */
#define GC_IO_PARTS 40
int32_t gc_pipeline_get_io_parts(gc_pipeline* p, double* h_parts);
int32_t gc_pipeline_get_io_evidence(gc_pipeline* p, double* h_L, double* h_h, double* h_cert);
int32_t gc_pipeline_set_iw(gc_pipeline* p, const double* h_nu_proc7, const double* h_Psi_proc7x36,
                           const double* h_nu_meas3, const double* h_Psi_meas3x9);
int32_t gc_pipeline_get_iw(gc_pipeline* p, double* h_nu_proc7, double* h_Psi_proc7x36, double* h_nu_meas3,
                           double* h_Psi_meas3x9, double* h_Q22x22, double* h_cert4);
int32_t gc_pipeline_set_map(gc_pipeline* p, const double* h_map);
int32_t gc_pipeline_get_map(gc_pipeline* p, double* h_map, double* h_map_der, double* h_misc2);
/* Staging (stage_scan / stage_pointcloud2 / stage_odom) is the per-scan ingest
 * (backend_node.py:1679-1690): the host arrays are copied into the slot's pinned mirror before the
 * call returns (the caller may reuse them at once), then DMA'd into HBM on the pipeline's copy
 * stream, ordered after the last scan that read the slot; scan_local waits for the slot's copy. So
 * staging scan k+1 into a second slot overlaps scan k's compute. The call blocks only while the
 * slot's previous DMA is still reading its pinned mirror. */
int32_t gc_pipeline_stage_scan(gc_pipeline* p, int32_t slot, const double* h_points, const double* h_t,
                               const double* h_w, int64_t n_in, const double* h_imu_t, const double* h_imu_gyro,
                               const double* h_imu_accel);
/* Stage a scan slot straight from a PointCloud2 message (the on-wire format): the raw bytes are
 * uploaded once and parsed on the device into the slot (gc_pointcloud2_parse layout of h_fields;
 * h_R9/h_t3 = T_base_lidar). An empty cloud stages one zero-weight dummy point, as the node does
 * (backend_node.py:1700-1707). */
int32_t gc_pipeline_stage_pointcloud2(gc_pipeline* p, int32_t slot, const uint8_t* h_data, int64_t n_points,
                                      int32_t point_step, const int32_t* h_fields, double header_stamp,
                                      const double* h_R9, const double* h_t3, const double* h_imu_t,
                                      const double* h_imu_gyro, const double* h_imu_accel);
/* Enqueue one scan (all local hypotheses, exchange, combine, IW apply, map update) =
 * gc_pipeline_scan_local + gc_pipeline_scan_finish(p, NULL). */
int32_t gc_pipeline_run_scan(gc_pipeline* p, int32_t slot, double scan_start, double scan_end, double t_last,
                             double t_scan, double dt_sec, int64_t scan_count);
/* The two halves of a scan around the per-scan exchange (backend_node.py:2036-2119):
 *  scan_local   a1-a15 for this rank's hypotheses and its partial record (partial_len doubles:
 *               weighted L/h/z/μ sums, IW statistics, hypothesis-0 map increment, anchor).
 *  get_partial  reads that record back (synchronises the stream).
 *  scan_finish  the exchange and the combine: with h_gather (world_size x partial_len doubles, in
 *               rank order, gathered by the caller over any transport) the records are uploaded;
 *               with NULL the pipeline all-gathers over its RCCL communicator (world_size > 1, or a
 *               single rank with one attached) or reads its own record (one rank, none attached).
 *               Then the fixed rank-order reduction, barycenter, IW apply, Q and map update.
 * Every rank ends the scan with a bit-identical combined belief, IW state and map.
 * Between the two halves the state the combine reads or writes is locked: set_bins / set_beliefs /
 * set_weights / set_io_evidence / set_io_mode / set_iw / set_map, get_combined / get_iw / get_map,
 * attach_comm and a second scan_local return GC_ERR_ARG. Allowed: get_partial, the per-hypothesis
 * getters (beliefs, diag, bin stats, hyp stats, io evidence: final after scan_local) and staging
 * the next scan into any slot (ordered after the pending scan's reads of it) except, with a
 * PrimitiveMap attached, the pending scan's own slot (its map update reads it in scan_finish). */
int32_t gc_pipeline_scan_local(gc_pipeline* p, int32_t slot, double scan_start, double scan_end, double t_last,
                               double t_scan, double dt_sec, int64_t scan_count);
int32_t gc_pipeline_partial_len(const gc_pipeline* p);
int32_t gc_pipeline_get_partial(gc_pipeline* p, double* h_record);
int32_t gc_pipeline_scan_finish(gc_pipeline* p, const double* h_gather);
/* LiDAR evidence source. GC_LIDAR_BINS (default): the legacy bin path, fused bins -> Matrix-Fisher ->
 * planar WLS inside the scan. GC_LIDAR_GIVEN: the reference's current scan step (backend/pipeline.py:
 * 778-1230), whose LiDAR evidence comes from the primitive map (surfels -> OT association ->
 * visual_pose_evidence -> L_lidar, :998-1015). The scan is then split around the caller's map branch:
 *  scan_front          predict and, per hypothesis, L_pred, the IMU/odom branch (:595-750) and the
 *                      linearisation pose z_lin_pose (:751-755). No bins run; the launch is the slot's last
 *                      reader and releases it for restaging.
 *  front_poses         device pointers (Hl,6) to z_lin_pose and pose_pred, valid until the next front
 *                      (get_front_poses downloads them, get_front_twists the deskew twists xi_body; in
 *                      GC_LIDAR_BINS pose_pred is the last scan's and z_lin_pose is not computed).
 *  set_lidar_evidence  L_lidar (Hl,22,22) and h_lidar (Hl,22) as DEVICE pointers on the pipeline's
 *                      context, copied device to device on its stream (stream order is the only
 *                      synchronisation with the launch that wrote them), and the LiDAR side's aggregated
 *                      certificate rows (host; copied through a pinned buffer on the same stream, so the
 *                      call does not wait for the device; cert_rows = 1 broadcasts one row, or Hl rows), GC_LIDAR_CERT
 *                      doubles each: [ess_total, support_frac, nll_per_ess, exc_dt, exc_ex, trigger_sum]
 *                      of aggregate_certificates([deskew, surfel, assoc, visual]) (:1056-1064); trigger_sum
 *                      is the sum of those operators' (and the recency inflation's) trigger magnitudes
 *                      (:1211). Without a map branch the evidence is eps_lift I, 0 (:1014-1015).
 *  scan_back           L_raw = L_io + L_lidar (:1038-1039), the combined certificate (:1065-1067),
 *                      tempering, excitation scaling, fusion, recompose, IW statistics, anchor drift
 *                      (:1070-1230) and the partial record; then get_partial / scan_finish as after
 *                      scan_local. The bin map is left bit for bit as it was (no forgetting step), the map
 *                      increment in the record is zero, and diag entries 18, 19 and 21:30 are 0.
 * GC_ERR_ARG: set_lidar_mode while a scan is under way or with a scan map attached (attaching one in
 * GC_LIDAR_GIVEN is refused too: that update is the bin path's; step 12b, :1236-1327, is the caller's
 * map update after the scan); scan_local / run_scan in GC_LIDAR_GIVEN; scan_front in GC_LIDAR_BINS or
 * before the previous front's back; set_lidar_evidence outside front..back; scan_back without a front or
 * without evidence; get_bin_stats / get_projection_certs in GC_LIDAR_GIVEN. Between front and back the
 * state is locked as between scan_local and scan_finish. */
#define GC_LIDAR_BINS 0
#define GC_LIDAR_GIVEN 1
#define GC_LIDAR_CERT 6
int32_t gc_pipeline_set_lidar_mode(gc_pipeline* p, int32_t mode);
int32_t gc_pipeline_scan_front(gc_pipeline* p, int32_t slot, double scan_start, double scan_end, double t_last,
                               double t_scan, double dt_sec, int64_t scan_count);
int32_t gc_pipeline_front_poses(gc_pipeline* p, const double** d_lin_pose, const double** d_pose_pred);
int32_t gc_pipeline_get_front_poses(gc_pipeline* p, double* h_lin_pose, double* h_pose_pred);
/* (Hl,6) deskew twists xi_body and (Hl) ESS of the scan-window IMU weights (DeskewConstantTwist's
 * ess_imu, pipeline.py:530-560) of the last predict launch, in either mode; either pointer may be NULL.
 * Like get_front_poses it is a plain read of the device buffers: before the first scan they hold zeros,
 * and between scans the last scan's values. */
int32_t gc_pipeline_get_front_twists(gc_pipeline* p, double* h_xi, double* h_ess_imu);
/* The one small download a step needs between front and back (the reference's own sync, pipeline.py:811):
 * local hypothesis 0's [xi_body 6 | ess_imu | pose_pred 6], three copies and one wait. GC_ERR_ARG without
 * an enqueued front. */
int32_t gc_pipeline_get_front_hyp0(gc_pipeline* p, double* h_out13);
int32_t gc_pipeline_set_lidar_evidence(gc_pipeline* p, const double* d_L, const double* d_h, const double* h_cert,
                                       int32_t cert_rows);
int32_t gc_pipeline_get_lidar_evidence(gc_pipeline* p, double* h_L, double* h_h, double* h_cert);
int32_t gc_pipeline_scan_back(gc_pipeline* p);
int32_t gc_pipeline_get_combined(gc_pipeline* p, double* h_out);
int32_t gc_pipeline_get_hyp_diag(gc_pipeline* p, double* h_diag);
/* Per-hypothesis ConditioningCert (Hl, 2, 4) of the last scan's two 22x22 PSD projections,
 * [L_pred (predict.py:183-188), L_post (fusion.py:150-230)] x [eig_min, eig_max, cond,
 * near_null_count] of the clamped spectrum. The scan certifies both by Cholesky and skips their
 * eigen-decompositions. With in-scan certificates on (gc_pipeline_set_inscan_certs) every scan
 * computes them right after its evidence kernel (Householder tridiagonalisation + Sturm
 * multisection, gc_certs.hip) and this getter reads them back; otherwise it computes them on demand
 * (Jacobi, off the scan path) from the stored matrices, so call it before the beliefs are set again.
 * Synchronises the stream. */
int32_t gc_pipeline_get_hyp_conditioning(gc_pipeline* p, double* h_out);
/* In-scan ConditioningCerts (off by default): on != 0 makes every later scan emit the certificates
 * gc_pipeline_get_hyp_conditioning reads, as the reference emits them on every predict / fusion call. */
int32_t gc_pipeline_set_inscan_certs(gc_pipeline* p, int32_t on);
/* The full certificate vector of every other PSD projection of the last scan, in the reference's
 * cert_vec layout [projection_delta, sym_delta, eig_min, eig_max, cond, near_null_count]
 * (domain_projection_psd_core, primitives.py:80-123; eigenvalues clamped at eps_psd, near-null =
 * clamped eigenvalues below 10 eps_psd), recomputed from the unprojected matrices by a full
 * eigen-decomposition (the scan certifies these projections by Cholesky and keeps only their deltas):
 *   h_hyp  (Hl, B + 2, 6): per hypothesis, GC_PCERT_BIN0 + b = the a6 Σ_p of bin b (binning.py:175-187),
 *          GC_PCERT_MF(B) = the a7 L_rot (matrix_fisher_evidence.py:330-331), GC_PCERT_PLANAR(B) = the
 *          a8 L_trans (matrix_fisher_evidence.py:609-610);
 *   h_scan (GC_PCERT_SCAN, 6): the a16 barycenter L (hypothesis.py:99), the 7 process-IW blocks
 *          (inverse_wishart_jax.py:168-172, each padded 6x6 block), the 3 measurement-IW blocks
 *          (measurement_noise_iw_jax.py:82-86) and Q (inverse_wishart_jax.py:67).
 * With in-scan certificates on, every scan computes them after its combine; otherwise this getter
 * does, from the last scan's stored matrices (call it before the next scan). Synchronises the stream. */
#define GC_PCERT_BIN0 0
#define GC_PCERT_MF(B) (B)
#define GC_PCERT_PLANAR(B) ((B) + 1)
#define GC_PCERT_SCAN 12
#define GC_PCERT_BARY 0
#define GC_PCERT_PROC0 1
#define GC_PCERT_MEAS0 8
#define GC_PCERT_Q 11
int32_t gc_pipeline_get_projection_certs(gc_pipeline* p, double* h_hyp, double* h_scan);
/* The a2 predict's route (predict.py:43-98). 0 (default): split at its first projection — when
 * Σ'_psd = Σ'_sym is certified, the predicted moments the bins need (μ_inc, σ_warp) are solved from Σ'
 * directly, (L_pred + ε_l I)⁻¹ L_pred = (I + ε_l(Σ' + ε_l I))⁻¹, and L_pred / h_pred / the predict cert
 * are formed in the bins launch beside the bin tasks; otherwise the factorised chain runs. 1: always the
 * factorised chain in the predict kernel (tests compare the two routes). */
int32_t gc_pipeline_set_predict_route(gc_pipeline* p, int32_t route);
/* L_evidence[pose, pose] (Hl, 6, 6) of the last scan, as the reference's MinimalScanTape.L_pose6
   (pipeline.py:1537). */
int32_t gc_pipeline_get_lpose6(gc_pipeline* p, double* h_lpose);
/* The last scan's bin statistics (Hl, B, GC_BIN_STATS), bin certificates (Hl, GC_BIN_CERT) and deskew
 * twists (Hl, 6) (any pointer may be NULL). Columns 4:13 of a row, the per-bin direction scatter
 * Σ r w d dᵀ, are computed only for global hypothesis 0 (h_begin + local index == 0) and are exactly 0.0
 * for every other hypothesis: in the scan their only reader is the bin map's increment, which global
 * hypothesis 0 alone feeds, so the other hypotheses' long bin tasks (32 iterations: 128 hypotheses and more at
 * 65,536 points) accumulate 13 of the 19 moment features, and the finalize writes the zeros whichever task
 * form ran. Every other column is computed for every hypothesis. gc_pipeline_set_bin_scatter_all brings the
 * scatter back for all of them. */
int32_t gc_pipeline_get_bin_stats(gc_pipeline* p, double* h_stats, double* h_cert, double* h_xi);
/* Per-bin direction scatter for every hypothesis (off by default): with on != 0 every later scan's bin
 * tasks accumulate all 19 moment features, and columns 4:13 of gc_pipeline_get_bin_stats are filled
 * for every hypothesis, at the cost of the larger feature set in long tasks (a diagnostic mode; the scan's beliefs
 * and map agree with the default's to rounding). */
int32_t gc_pipeline_set_bin_scatter_all(gc_pipeline* p, int32_t on);
/* Per-hypothesis statistics of the last scan (any pointer may be NULL): process-IW sufficient
 * statistics dPsi (Hl,7,6,6) and measurement-IW dPsi (Hl,3,3,3) before the weighted accumulation
 * (backend_node.py:2085-2090), and the covariance of each updated belief Σ = (L + ε_lift I)⁻¹
 * (Hl,22,22) (BeliefGaussianInfo covariance, belief.py:373-386). */
int32_t gc_pipeline_get_hyp_stats(gc_pipeline* p, double* h_dPsi_proc, double* h_dPsi_meas, double* h_Sigma);
int32_t gc_pipeline_attach_comm(gc_pipeline* p, gc_comm* comm);
/* Size of the attached RCCL communicator (0 when none is attached). */
int32_t gc_pipeline_comm_size(const gc_pipeline* p);
/* Exchange timing (off by default): with on != 0, every later scan's exchange is bracketed by two
 * HIP events on the pipeline stream (each event between kernels costs the stream a few us, so the
 * timed product loop leaves it off). */
int32_t gc_pipeline_set_exchange_timing(gc_pipeline* p, int32_t on);
/* Device time (ms) of the last timed scan's exchange: the RCCL all-gather of the partial records,
 * or the upload of the host-gathered records. Synchronises on it. GC_ERR_ARG when no timed
 * exchange has run (timing off, or one rank without a communicator). */
int32_t gc_pipeline_exchange_ms(gc_pipeline* p, float* ms);

/* Per-stage device timing (off by default; the reference fills MinimalScanTape.t_*_ms per stage,
 * pipeline.py:383-394, :1560-1569). With on != 0 every later scan records GC_STAGE_N HIP events on the
 * pipeline stream, before predict and after each launch group; gc_pipeline_stage_ms returns the last
 * finished scan's stage times (ms) [predict (a1 scalars, a2, a3), bins (a1 selection, a4, a5, a6 and
 * the IMU/odom branch, + finalize), evidence (a7-a15), combine_local, exchange, combine_final (a16, IW
 * apply, bin-map update), map_update (the attached PrimitiveMap's, 0 without one), total]. Each event
 * between kernels costs the stream ~1-5 us, so the timed product loop leaves it off. stage_ms
 * synchronises on the last event. In GC_LIDAR_GIVEN the stages keep their indices: "bins" is the front's
 * second launch (L_pred, IMU/odom branch, z_lin_pose), and "evidence" runs from its end to the end of the
 * evidence launch, so it includes whatever the caller enqueued on the stream between front and back. */
#define GC_STAGE_N 8
int32_t gc_pipeline_set_stage_timing(gc_pipeline* p, int32_t on);
int32_t gc_pipeline_stage_ms(gc_pipeline* p, float* h_ms_out);
/* Host-side accounting since creation or the last reset (GC_HOST_STATS doubles): the reference's
 * RuntimeCounters / DeviceRuntimeCert (common/runtime_counters.py:19-108, backend_node.py:2182-2190:
 * host syncs, host->device and device->host bytes, JIT recompiles = 0 for this AOT library), and the
 * split of the host time of every scan (scan_local + scan_finish) and every staging call into its
 * own work (argument checks, pinned copies, launch / DMA enqueue) and its waits on the device (slot
 * events, stream syncs). Times in ms. reset != 0 zeroes the counters after reading them. */
#define GC_HOST_STATS 16
#define GC_HS_SCANS 0
#define GC_HS_SCAN_ENQ_MS 1
#define GC_HS_SCAN_ENQ_MAX 2
#define GC_HS_SCAN_WAIT_MS 3
#define GC_HS_SCAN_WAIT_MAX 4
#define GC_HS_STAGES 5
#define GC_HS_STAGE_WORK_MS 6
#define GC_HS_STAGE_WORK_MAX 7
#define GC_HS_STAGE_WAIT_MS 8
#define GC_HS_STAGE_WAIT_MAX 9
#define GC_HS_HOST_SYNCS 10
#define GC_HS_H2D_BYTES 11
#define GC_HS_D2H_BYTES 12
#define GC_HS_JIT_RECOMPILES 13
int32_t gc_pipeline_host_stats(gc_pipeline* p, double* h_out, int32_t reset);

/* The C5 in-scan PrimitiveMap update (config C5; the reference's step 12b, pipeline.py:1236-1327,
 * transform_gaussian_to_world :1248-1256 + primitive_map_fuse, primitive_map.py:992-1163).
 * BUILD-DEFINED, parity unpinned (csrc/gc_scanmap.hip): with a map attached,
 * scan_finish fuses every budgeted point of the scan, deskewed with hypothesis 0's twist, as one
 * world-frame Gaussian row (pose z_t of hypothesis 0 with t_z = 0, covariance Σ_lidar inflated by
 * J Σ_pose Jᵀ) into the slot hashed from its voxel (edge voxel_m), responsibility 1, source
 * LiDAR, timestamp scan_end, scan_seq = scan_count. Σ_lidar is the measurement-IW LiDAR mode of the
 * state the scan started from (before its own IW apply). Which ranks run it is the scan-map mode
 * (gc_pipeline_set_scan_map_mode): by default only the rank whose shard holds hypothesis 0 (the
 * reference's owner, backend_node.py:2081-2083); replicated, every rank runs it from the reduced
 * record and the replicas stay bit-identical. The map's device arrays must outlive the attachment;
 * map == NULL detaches. */
struct gc_primitive_map; /* defined with the PrimitiveMap entries below */
int32_t gc_pipeline_attach_primitive_map(gc_pipeline* p, const struct gc_primitive_map* map, double voxel_m);
#define GC_SMAP_OWNER 0      /* default: the update runs on hypothesis 0's rank only */
#define GC_SMAP_REPLICATED 1 /* every rank updates its replica of the map */
/* Not while a scan is pending. A pipeline with world size 1 holds hypothesis 0: both modes update. */
int32_t gc_pipeline_set_scan_map_mode(gc_pipeline* p, int32_t mode);
/* The attached map's colour fields were written outside the pipeline (an insert, a merge, a colour
 * upload): the next in-scan update recomputes rgb / colors on every slot, as primitive_map_fuse does
 * on every fuse (primitive_map.py:1097-1105); while they stay current it only touches its rows' slots.
 * Allowed while a scan is pending (the pass then runs in that scan's finish). */
int32_t gc_pipeline_map_colors_stale(gc_pipeline* p);
/* Hypothesis 0's [z_t 6, Σ_post pose block 36 (row-major 6x6), ξ_body 6] that the last scan's
 * update used (from the reduced record). */
int32_t gc_pipeline_get_scan_map_pose(gc_pipeline* p, double* h_out48);
/* Distinct map slots the last in-scan update touched (synchronises the stream); 0 on a rank that does
 * not run the update. */
int32_t gc_pipeline_get_scan_map_count(gc_pipeline* p, int64_t* n_slots);

/* ------------------------------------------------------------------ RCCL communicator */
#define GC_COMM_ID_BYTES 128
int32_t gc_comm_unique_id(uint8_t* h_id_out);
int32_t gc_comm_init(gc_ctx* ctx, int32_t nranks, int32_t rank, const uint8_t* h_id, gc_comm** out);
int32_t gc_comm_destroy(gc_comm* comm);
/* Abort the communicator (ncclCommAbort: its kernels exit; every later exchange fails fast). The
 * bounded waits of the context it was created on call this themselves on a timeout or an RCCL error. */
int32_t gc_comm_abort(gc_comm* comm);
/* *ok = 0 when the communicator has an asynchronous error or was aborted (gc_last_error has why). */
int32_t gc_comm_healthy(gc_comm* comm, int32_t* ok);
int32_t gc_comm_allgather_f64(gc_ctx* ctx, gc_comm* comm, const double* d_send, double* d_recv, int64_t count);

/* ------------------------------------------------------------------------------------------
 * Per-operator entries: each reference operator of the hot path as one launch over H
 * independent items (the gcslam.ops mirror calls them with H = 1 at the reference's
 * per-hypothesis call sites). Matrices are row-major f64; "belief" arrays are
 * X_anchor (H,6), z_lin (H,22), L (H,22,22), h (H,22). The same device code runs inside the
 * batched pipeline above.
 * ------------------------------------------------------------------------------------------ */
#define GC_PRED_CERT 8      /* [lift, psd_delta, eig_min, eig_max, cond, nnc, trace_cov, trigger] */
#define GC_PREINT_OUT 32    /* [delta_pose 6, delta_R 9, p_body 3, v_body 3, ess, a_body_mean 3,
                               a_world_nog_mean 3, a_world_mean 3, dt_eff_sum] */
#define GC_MF_OUT 66        /* [R_mf 9, L_rot 9, h_rot 3, delta_rot 3, svd 3, N_eff, nll_per_ess, psd_delta,
                               trigger, nll, map scatter 17, scan scatter 17]; scatter = [eigenvalues 3
                               (descending), eigenvectors 9 (row-major, columns = vectors), linearity,
                               planarity, sphericity, anisotropy, effective_rank] */
#define GC_PT_OUT 26        /* [t_wls 3, L_trans 9, h_trans 3, delta_trans 3, z_scale, N_eff, nll_per_ess,
                               psd_delta, trigger, xy_info_scale, z_info_scale, nll] */
#define GC_RECOMPOSE_OUT 19 /* [delta_pose 6, X_new 6, frobenius_strength, bch_correction 6] */
#define GC_DRIFT_OUT 3      /* [rho, drift_m, drift_r] */
#define GC_FUSION_ROW 8     /* in: [cond, ess_total, support_frac, excitation_total, dt_asymmetry,
                               z_to_xy_ratio, power_beta, nll_per_ess] */
#define GC_FUSION_OUT 4     /* [alpha, excitation_total, ess_to_excitation, cond_to_support] */
#define GC_BARY_CERT 16     /* [floor_adjustment, spread, ess, support_frac, mass_eps, psd cert 6, pad 5] */

/* IMU/odom-branch factors (pipeline.py:595-776), one thread per item.
 * Item rows: d_in (H, GC_IOF_IN) per kind below; d_out (H, GC_IOF_OUT) = L (22,22) | h (22) |
 * extras (16). Each kind replaces one reference operator:
 *  GC_IOF_ODOM_QUADRATIC    odom_quadratic_evidence (odom_evidence.py:87-154)
 *     in [pose_pred 6, odom_pose 6, cov 36, eps_psd, eps_lift]
 *     ex [delta_z_pose 6, nll, lift, eig_min, eig_max, cond, nnc]
 *  GC_IOF_IMU_GYRO_ROTATION imu_gyro_rotation_evidence (imu_gyro_evidence.py:103-163)
 *     in [rv_start 3, rv_end_pred 3, delta_rotvec 3, Sigma_g 9, dt_int, eps_psd, eps_lift, eps_mass]
 *     ex [r_rot 3, nll, lift, eig_min, eig_max, nnc]
 *  GC_IOF_IMU_PREINT_FACTOR imu_preintegration_factor (imu_preintegration_factor.py:46-180)
 *     in [p_start 3, rv_start 3, v_start 3, p_end_pred 3, v_end_pred 3, delta_v_body 3,
 *         delta_p_body 3, Sigma_a 9, dt_int, eps_psd, eps_lift, eps_mass]
 *     ex [r_vel 3, r_pos 3, nll, lift, eig_min, eig_max, cond, nnc]
 *  GC_IOF_PLANAR_Z_PRIOR    planar_z_prior (planar_prior.py:55-135): in [pose 6, z_ref, sigma_z]; ex [r_z, nll]
 *  GC_IOF_VELOCITY_Z_PRIOR  velocity_z_prior (planar_prior.py:138-195): in [v_z, sigma_vz]; ex [v_z, nll]
 *  GC_IOF_ODOM_VELOCITY     odom_velocity_evidence (odom_twist_evidence.py:58-154)
 *     in [v_pred_world 3, R_world_body 9, v_odom_body 3, Sigma_v 9, eps_psd, eps_lift]
 *     ex [r_vel 3, nll, lift, eig_min, eig_max, cond, nnc]
 *  GC_IOF_ODOM_YAWRATE      odom_yawrate_evidence (odom_twist_evidence.py:157-225)
 *     in [omega_z_pred, omega_z_odom, sigma_wz]; ex [r_wz, nll]
 *  GC_IOF_KINEMATIC         pose_twist_kinematic_consistency (odom_twist_evidence.py:251-397)
 *     in [pose_prev 6, pose_curr 6, v_body 3, omega_body 3, dt, Sigma_v 9, Sigma_omega 9, eps_psd, eps_lift]
 *     ex [r_trans 3, r_rot 3, nll, lift, eig_min, eig_max, cond]
 *  GC_IOF_IMU_DEPENDENCE    imu_dependence_inflation (imu_evidence.py:562-589): in [transport_sigma, eps_mass]; ex [scale]
 *  GC_IOF_ODOM_DEPENDENCE   odom_dependence_inflation (odom_twist_evidence.py:400-430):
 *     in [r_trans 3, r_rot 3, eps_mass]; ex [scale] */
#define GC_IOF_IN 64
#define GC_IOF_OUT (484 + 22 + 16)
#define GC_IOF_ODOM_QUADRATIC 0
#define GC_IOF_IMU_GYRO_ROTATION 1
#define GC_IOF_IMU_PREINT_FACTOR 2
#define GC_IOF_PLANAR_Z_PRIOR 3
#define GC_IOF_VELOCITY_Z_PRIOR 4
#define GC_IOF_ODOM_VELOCITY 5
#define GC_IOF_ODOM_YAWRATE 6
#define GC_IOF_KINEMATIC 7
#define GC_IOF_IMU_DEPENDENCE 8
#define GC_IOF_ODOM_DEPENDENCE 9
#define GC_IOF_NKINDS 10
int32_t gc_io_factor_batch(gc_ctx* ctx, int32_t kind, int32_t H, const double* d_in, double* d_out);
/* imu_vmf_gravity_evidence_time_resolved (imu_evidence.py:402-559), one workgroup per item over
 * the shared IMU window accel/gyro (M,3); rotvec (H,3), weights (H,M), accel_bias (H,3), g3 host.
 * d_out (H, GC_IOF_OUT), ex = [kappa, ess_weighted, ess_raw, mean_reliability, transport_sigma,
 * Rbar, nll, nll_per_ess, psd_delta, eig_min, eig_max, cond, nnc, xbar 3]. */
int32_t gc_imu_vmf_gravity_tr_batch(gc_ctx* ctx, int32_t H, int32_t M, const double* d_rotvec, const double* d_accel,
                                    const double* d_gyro, const double* d_w, const double* d_ba, const double* g3,
                                    double dt_imu, double eps_psd, double eps_mass, double* d_out);

/* SO(3)/SE(3) maps of common/geometry/se3_jax.py, batched: n items of the op's input row
 * (d_in (n, in)) to its output row (d_out (n, out)), one thread per item. These are the device
 * routines every kernel of the scan path uses (recompose, world pose, ξ_body, MF δ, IMU/odom
 * residuals). Rotations are row-major 3x3; poses [t 3, rotvec 3]; twists [ρ 3, φ 3].
 *   GC_LIE_SO3_EXP     so3_exp      (se3_jax.py:259-301)   in 3  out 9
 *   GC_LIE_SO3_LOG     so3_log      (se3_jax.py:304-366)   in 9  out 3  (softmax near-π axis)
 *   GC_LIE_SE3_EXP     se3_exp      (se3_jax.py:473-504)   in 6  out 6
 *   GC_LIE_SE3_LOG     se3_log      (se3_jax.py:220-256)   in 6  out 6
 *   GC_LIE_SE3_V       se3_V        (se3_jax.py:137-175)   in 3  out 9
 *   GC_LIE_SE3_V_INV   _se3_V_inv   (se3_jax.py:177-217)   in 3  out 9
 *   GC_LIE_SE3_COMPOSE se3_compose  (se3_jax.py:420-438)   in 12 (a, b) out 6
 *   GC_LIE_SE3_INVERSE se3_inverse  (se3_jax.py:441-453)   in 6  out 6 */
#define GC_LIE_SO3_EXP 0
#define GC_LIE_SO3_LOG 1
#define GC_LIE_SE3_EXP 2
#define GC_LIE_SE3_LOG 3
#define GC_LIE_SE3_V 4
#define GC_LIE_SE3_V_INV 5
#define GC_LIE_SE3_COMPOSE 6
#define GC_LIE_SE3_INVERSE 7
#define GC_LIE_NOPS 8
int32_t gc_lie_batch(gc_ctx* ctx, int32_t op, int64_t n, const double* d_in, double* d_out);

/* spd_cholesky_inverse_lifted_core (common/primitives.py:169-192): d_out = (L + eps_lift I)⁻¹ for H
 * n x n SPD matrices (n <= 22), by the Cholesky factor and C⁻ᵀ C⁻¹ as in the batched pipeline. */
int32_t gc_spd_inverse_lifted_batch(gc_ctx* ctx, int32_t H, int32_t n, const double* d_L, double eps_lift,
                                    double* d_out);
/* BeliefGaussianInfo.mean_increment + world pose X ∘ Exp(δz) (common/belief.py:373-425). */
int32_t gc_belief_world_pose_batch(gc_ctx* ctx, int32_t H, const double* d_X, const double* d_L, const double* d_h,
                                   double eps_lift, double* d_pose_out, double* d_mean_out);
/* predict_diffusion (backend/operators/predict.py:106-214 -> core :43-98); Q (22,22) shared. */
int32_t gc_predict_diffusion_batch(gc_ctx* ctx, int32_t H, const double* d_L, const double* d_h, const double* d_Q,
                                   double dt_sec, double eps_psd, double eps_lift, double lambda_ou, double* d_L_out,
                                   double* d_h_out, double* d_cert_out);
/* smooth_window_weights (backend/operators/imu_preintegration.py:20-43). */
int32_t gc_smooth_window_weights(gc_ctx* ctx, int32_t M, const double* d_stamps, double t0, double t1, double sigma,
                                 double* d_w_out);
/* preintegrate_imu_relative_pose_jax (imu_preintegration.py:47-147); M <= 512 samples shared by
   the H items; weights (H, weights_stride) or shared (stride 0); rotvec0/biases (H,3);
   h_gravity3 NULL = (0, 0, -9.81). out (H, GC_PREINT_OUT). */
int32_t gc_preintegrate_imu_batch(gc_ctx* ctx, int32_t H, int32_t M, const double* d_stamps, const double* d_gyro,
                                  const double* d_accel, const double* d_weights, int64_t weights_stride,
                                  const double* d_rotvec0, const double* d_gyro_bias, const double* d_accel_bias,
                                  const double* h_gravity3, double* d_out);
/* imu_gyro_meas_iw_suffstats_from_avg_rate_jax + imu_accel_meas_iw_suffstats_from_gravity_dir_jax
   (measurement_noise_iw_jax.py:131-218); out (H, 18) = [dPsi_gyro 9, dPsi_accel 9]. */
int32_t gc_imu_meas_iw_suffstats_batch(gc_ctx* ctx, int32_t H, int32_t M, const double* d_gyro, const double* d_accel,
                                       const double* d_weights, const double* d_gyro_bias, const double* d_accel_bias,
                                       const double* d_omega_avg, const double* d_rotvec0, double dt_imu,
                                       double eps_mass, double eps_psd, double* d_out);
/* matrix_fisher_rotation_evidence (archive/legacy_operators/matrix_fisher_evidence.py:264-394):
   pose_pred (H,6) = world pose of belief_pred; scan (H,B,*), map (B,*); scatter inputs may be
   NULL (metrics then use zero scatter). out (H, GC_MF_OUT). */
int32_t gc_matrix_fisher_batch(gc_ctx* ctx, int32_t H, int32_t B, const double* d_pose_pred, const double* d_scan_s_dir,
                               const double* d_scan_N, const double* d_scan_S_dir_scatter, const double* d_map_S_dir,
                               const double* d_map_N_dir, const double* d_map_S_dir_scatter, double eps_psd,
                               double eps_mass, double* d_out);
/* planar_translation_evidence (matrix_fisher_evidence.py:502-671); R_hat (H,9); out (H, GC_PT_OUT). */
int32_t gc_planar_translation_batch(gc_ctx* ctx, int32_t H, int32_t B, const double* d_pose_pred, const double* d_R_hat,
                                    const double* d_scan_p_bar, const double* d_scan_Sigma_p, const double* d_scan_N,
                                    const double* d_map_centroid, const double* d_map_Sigma_c,
                                    const double* d_map_N_pos, const double* d_map_S_dir_scatter,
                                    const double* d_map_N_dir, double eps_psd, double eps_mass, double* d_out);
/* compute_excitation_scales_jax + apply_excitation_prior_scaling_jax (backend/operators/excitation.py:15-64);
   s_out (H,2) = [s_dt, s_ex]. With d_L_ev == NULL, s_out is an input and only the scaling is applied. */
int32_t gc_excitation_scaling_batch(gc_ctx* ctx, int32_t H, const double* d_L_ev, const double* d_L_prior,
                                    const double* d_h_prior, double eps, double* d_s_out, double* d_L_out,
                                    double* d_h_out);
/* fusion_scale_from_certificates (backend/operators/fusion.py:46-142) over H certificate rows. */
int32_t gc_fusion_scale_batch(gc_ctx* ctx, int32_t H, const double* d_rows, double alpha_min, double alpha_max,
                              double c0_cond, double eps_mass, double* d_out);
/* info_fusion_additive (backend/operators/fusion.py:150-230); alpha (H); cert (H,6) PSD cert. */
int32_t gc_info_fusion_additive_batch(gc_ctx* ctx, int32_t H, const double* d_L_pred, const double* d_h_pred,
                                      const double* d_L_ev, const double* d_h_ev, const double* d_alpha,
                                      double eps_psd, double* d_L_out, double* d_h_out, double* d_cert_out);
/* pose_update_frobenius_recompose (backend/operators/recompose.py:94-205); T (H). */
int32_t gc_recompose_batch(gc_ctx* ctx, int32_t H, const double* d_X, const double* d_z, const double* d_L,
                           const double* d_h, const double* d_T, double c_frob, double eps_lift, double* d_X_out,
                           double* d_z_out, double* d_h_out, double* d_res_out);
/* anchor_drift_update (backend/operators/anchor_drift.py:93-191). */
int32_t gc_anchor_drift_batch(gc_ctx* ctx, int32_t H, const double* d_X, const double* d_z, const double* d_L,
                              const double* d_h, double eps_lift, double* d_X_out, double* d_z_out, double* d_h_out,
                              double* d_res_out);
/* process_noise_iw_suffstats_from_info_jax (inverse_wishart_jax.py:72-123): dPsi (H,7,6,6), dnu (H,7). */
int32_t gc_iw_process_suffstats_batch(gc_ctx* ctx, int32_t H, const double* d_L_pred, const double* d_h_pred,
                                      const double* d_L_post, const double* d_h_post, double eps_lift,
                                      double* d_dPsi_out, double* d_dnu_out);
/* process_noise_iw_apply_suffstats_jax (inverse_wishart_jax.py:127-185): nu (7), Psi (7,6,6);
   cert (2) = [psd_delta sum, nu projection sum]. Outputs may alias the inputs. */
int32_t gc_iw_process_apply(gc_ctx* ctx, const double* d_nu, const double* d_Psi, const double* d_dPsi,
                            const double* d_dnu, double eps_psd, double nu_max, double* d_nu_out, double* d_Psi_out,
                            double* d_cert_out);
/* process_noise_state_to_Q_jax (inverse_wishart_jax.py:36-68): Q (22,22). */
int32_t gc_iw_process_Q(gc_ctx* ctx, const double* d_nu, const double* d_Psi, double eps_psd, double* d_Q_out);
/* measurement_noise_apply_suffstats_jax (measurement_noise_iw_jax.py:60-100): nu (3), Psi (3,3,3). */
int32_t gc_iw_meas_apply(gc_ctx* ctx, const double* d_nu, const double* d_Psi, const double* d_dPsi,
                         const double* d_dnu, double eps_psd, double nu_max, double* d_nu_out, double* d_Psi_out,
                         double* d_cert_out);
/* hypothesis_barycenter_projection (backend/operators/hypothesis.py:125-236 -> core :52-122). */
int32_t gc_hypothesis_barycenter(gc_ctx* ctx, int32_t H, const double* d_L, const double* d_h, const double* d_z,
                                 const double* d_weights, double weight_floor, double eps_psd, double eps_lift,
                                 double* d_L_out, double* d_h_out, double* d_z_out, double* d_cert_out);

/* ------------------------------------------------------------------------------------------
 * C5 map update (a13 C5 analogue): transform_gaussian_to_world (backend/pipeline.py:1248-1256)
 * fused into primitive_map_fuse (backend/structures/primitive_map.py:992-1163). The map is one
 * flat tile of m_slots slots in device memory; tile t / local slot j of the reference map to slot
 * t * m_tile + j. Two layouts:
 *   slot_bytes = 0  the reference's per-field arrays (SoA, row-major per slot): slot s of a field
 *                   of width w at field + s * w;
 *   slot_bytes > 0  one packed record per slot (gc_primitive_map_record_layout): every field
 *                   pointer is the record array plus the field's offset, slot s of every field at
 *                   (char*)field + s * slot_bytes. The fuse's read-modify-write fields share the
 *                   record's first two 128-B lines, so a touched slot moves 2 lines each way
 *                   instead of one partial line per field.
 * Colour fields are all NULL (no camera colour tracking) or all set. All pointers inside the
 * structs are device pointers.
 * ------------------------------------------------------------------------------------------ */
typedef struct gc_primitive_map {
  int64_t m_slots;
  int32_t n_lobes;          /* GC_VMF_N_LOBES (3) */
  /* 1 when every slot's rgb and colors already equal the fuse's colour estimate of its camera
     accumulators (the state a fuse leaves): the fuse then recomputes the colour of the slots it
     touches only, which gives the same map as the reference's all-slot recompute
     (primitive_map.py:1090-1098). 0: the fuse recomputes every slot. */
  int32_t colors_current;
  double* Lambdas;          /* (M, 3, 3) */
  double* thetas;           /* (M, 3) */
  double* etas;             /* (M, n_lobes, 3) */
  double* weights;          /* (M) */
  double* timestamps;       /* (M) */
  int64_t* last_supported_scan_seq;  /* (M) */
  int64_t* last_update_scan_seq;     /* (M) */
  double* cam_mass;         /* (M) or NULL */
  double* lidar_mass;       /* (M) or NULL */
  double* rgb_cam_accum;    /* (M, 3) or NULL */
  double* rgb_cam_denom;    /* (M) or NULL */
  double* rgb;              /* (M, 3) or NULL */
  double* colors;           /* (M, 3) or NULL */
  /* maintenance fields (primitive_map_insert_masked / cull / recency / merge; the fuse ignores
     them): valid_mask is required by those entries, the other two may be NULL */
  uint8_t* valid_mask;      /* (M) */
  double* created_timestamps;        /* (M) or NULL */
  int64_t* primitive_ids;            /* (M) or NULL */
  int64_t slot_bytes;                /* 0 = per-field arrays; else the packed record's size */
} gc_primitive_map;

/* Packed slot record for n_lobes lobes (build-defined device layout; the reference's per-field
   arrays are honoured at upload / download through gc_copy_strided). offsets_out (host, 16) =
   byte offsets of Lambdas, thetas, etas, weights, timestamps, last_supported_scan_seq,
   last_update_scan_seq, cam_mass, lidar_mass, rgb_cam_accum, rgb_cam_denom, rgb, colors,
   valid_mask, created_timestamps, primitive_ids (the struct's field order); *slot_bytes_out = the
   record size, a multiple of 128 B. */
int32_t gc_primitive_map_record_layout(int32_t n_lobes, int64_t* offsets_out, int64_t* slot_bytes_out);
/* rows x elem_bytes copied between device buffers with the given pitches (bytes; pitch >=
   elem_bytes, elem_bytes a multiple of 1, rows >= 0): the transposes between a packed map and
   per-field arrays. Asynchronous on the context's stream. */
int32_t gc_copy_strided(gc_ctx* ctx, void* d_dst, int64_t dst_pitch, const void* d_src, int64_t src_pitch,
                        int64_t elem_bytes, int64_t rows);

typedef struct gc_fuse_batch {
  int64_t K;
  const int32_t* target_slots;      /* (K) slot per row; out-of-range rows are dropped */
  const double* Lambdas;            /* (K, 3, 3) body (or world) frame */
  const double* thetas;             /* (K, 3) */
  const double* etas;               /* (K, n_lobes, 3) */
  const double* weights;            /* (K) */
  const double* responsibilities;   /* (K) */
  const uint8_t* valid_mask;        /* (K) or NULL = all valid */
  const double* colors;             /* (K, 3) or NULL */
  const int32_t* sources;           /* (K) 0 = camera, 1 = lidar, or NULL */
} gc_fuse_batch;

/* Fuse K rows into the map in place. h_pose6 (host, [t, rotvec]) = world pose z_t of the
   pushforward, or NULL when the rows are already in the world frame. n_fused_out (host, may be
   NULL) = number of distinct in-range slots touched; it synchronises the stream. */
int32_t gc_primitive_map_fuse(gc_ctx* ctx, const gc_primitive_map* map, const gc_fuse_batch* meas,
                              const double* h_pose6, double eps_lift, double eps_mass, double timestamp,
                              int64_t scan_seq, int64_t* n_fused_out);

/* ------------------------------------------------------------------------------------------
 * PrimitiveMap maintenance. Each entry works on one reference tile: the slot
 * range [slot0, slot0 + n_slots) of the flat map (tile t -> slot0 = t * m_tile). Reductions are
 * fixed-order (no float atomics); host outputs synchronise the stream.
 * ------------------------------------------------------------------------------------------ */
/* primitive_map_forget (primitive_map.py:1314-1390): weights *= gamma on every slot. */
int32_t gc_primitive_map_forget(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                                double gamma);
/* primitive_map_recency_inflate (primitive_map.py:1400-1490) on one tile: decay =
   clip(exp(-lambda max(0, scan_seq - last_supported)), min_scale, 1) on valid slots (1 elsewhere);
   Lambdas, thetas *= decay. h_stats3 (host, may be NULL) = [n_valid, sum (1 - decay), sum (1/decay - 1)]
   over valid slots. */
int32_t gc_primitive_map_recency_inflate(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                                         int64_t scan_seq, double decay_lambda, double min_scale,
                                         double* h_stats3);
/* primitive_map_cull (primitive_map.py:1175-1305): clears valid on valid slots with weight <
   threshold; with max_primitives >= 0 (< 0 = None) and more survivors than that, the threshold
   becomes the (max_primitives+1)-th largest of weight*valid. h_out4 (host) = [n_culled,
   mass_dropped, sum of all tile weights, n_valid before]. */
int32_t gc_primitive_map_cull(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                              double weight_threshold, int64_t max_primitives, double* h_out4);

typedef struct gc_insert_batch {
  int64_t K;
  const double* Lambdas;            /* (K, 3, 3) */
  const double* thetas;             /* (K, 3) */
  const double* etas;               /* (K, n_lobes, 3) */
  const double* weights;            /* (K) */
  const uint8_t* valid_mask;        /* (K) proposals with 0 are ignored */
  const double* colors;             /* (K, 3) or NULL (zeros) */
  const int32_t* sources;           /* (K) 0 = camera, 1 = lidar, or NULL (all lidar) */
} gc_insert_batch;

/* primitive_map_insert_masked (primitive_map.py:807-982): proposal k goes to the k-th slot of the
   tile ordered by retention key (valid ? w exp(-lambda max(0, seq - last_supported)) : -inf),
   ties by slot (_select_lowest_mass_slots_fixed :325-353, a stable sort on the key). Inserted
   proposals get ids next_global_id + (number inserted before them). d_target_slots_out (K, tile-
   local) and d_new_ids_out (K, -1 where not inserted) may be NULL. h_out2 (host) = [n_inserted,
   valid count of the tile after]. Requires 1 <= K <= n_slots. */
int32_t gc_primitive_map_insert_masked(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                                       const gc_insert_batch* batch, double timestamp, int64_t scan_seq,
                                       double recency_decay_lambda, int64_t next_global_id,
                                       int32_t* d_target_slots_out, int64_t* d_new_ids_out, int64_t* h_out2);
/* primitive_map_merge_reduce (primitive_map.py:1809-2030 -> _merge_reduce_jax :1501-1807):
   Bhattacharyya distances of all slot pairs i < j (+inf unless both valid), a stable ascending
   sort, greedy disjoint selection of up to max_pairs pairs with finite distance < threshold, and
   moment-matched merges into the lower slot. The caller applies the reference's tile-size cap.
   h_out2 (host) = [n_merged, valid count after]. Requires n_slots <= 65536. */
int32_t gc_primitive_map_merge_reduce(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                                      double merge_threshold, int32_t max_pairs, double eps_psd, double eps_lift,
                                      int64_t* h_out2);

/* ------------------------------------------------------------------------------------------
 * The post-pose map update (backend/pipeline.py:1232-1392, step 12b): the fuse of the N x K
 * associated rows into the active tiles, then the per-tile novelty insert, with no host wait
 * between the first launch and the last insert.
 *
 * Bounds (the insert plan keeps one workgroup's scores, in-tile flags and proposals in LDS:
 * 13 B per measurement row and 13 B per proposal of the CU's 160 KiB):
 *   1 <= N <= GC_MAP_UPDATE_MAX_ROWS, 1 <= k_insert <= min(N, m_tile, GC_MAP_UPDATE_MAX_INSERT),
 *   1 <= n_active <= GC_MAP_UPDATE_MAX_ACTIVE, 1 <= K <= GC_MAP_UPDATE_MAX_K.
 * ------------------------------------------------------------------------------------------ */
#define GC_MAP_UPDATE_MAX_ROWS 8192
#define GC_MAP_UPDATE_MAX_INSERT 1024
#define GC_MAP_UPDATE_MAX_ACTIVE 64
#define GC_MAP_UPDATE_MAX_K 64
/* per-call statistics (device doubles): [0] fused_mass_total, [1] sum over blocks of the distinct
   in-range slot numbers of the block (n_fused = n_active x this), [2..3] unused, then per active
   tile a at GC_MAP_UPDATE_STATS_HEAD + GC_MAP_UPDATE_STATS_TILE * a: [0] valid count of the tile
   after its insert, [1] n_inserted, [2] sum of weights_ins, [3] sorted weights_ins at the p95 index,
   [4] measurement rows in the tile, [5] 1 when the placeholder rule applied */
#define GC_MAP_UPDATE_STATS_HEAD 4
#define GC_MAP_UPDATE_STATS_TILE 8

/* The measurement batch (measurement_batch.py:68-134) and the association result
   (primitive_association.py:71-92), all in device memory, and the active tiles: their keys
   (device) and the dense tile of each in the map (device and host copies of the same list). */
typedef struct gc_map_update_in {
  int64_t N;                          /* measurement rows */
  int64_t m_tile;                     /* slots per tile: tile d = slots [d * m_tile, (d + 1) * m_tile) */
  int32_t K;                          /* candidates per row */
  int32_t n_active;
  int32_t k_insert;                   /* K_INSERT_TILE */
  int32_t block_size;                 /* GC_ASSOC_BLOCK_SIZE */
  const double* Lambdas;              /* (N, 3, 3) body frame */
  const double* thetas;               /* (N, 3) */
  const double* etas;                 /* (N, n_lobes, 3) */
  const double* weights;              /* (N) */
  const uint8_t* valid_mask;          /* (N) */
  const double* colors;               /* (N, 3) */
  const int32_t* sources;             /* (N) 0 = camera, 1 = lidar */
  const double* responsibilities;     /* (N, K) */
  const int64_t* candidate_tile_ids;  /* (N, K) tile keys */
  const int64_t* candidate_slots;     /* (N, K) tile-local slots */
  const double* row_masses;           /* (N) */
  const int64_t* active_keys;         /* (n_active) device */
  const int32_t* active_dense;        /* (n_active) device */
  const int32_t* h_active_dense;      /* (n_active) host: distinct, each in [0, m_slots / m_tile) */
} gc_map_update_in;

/* Device outputs, each (n_active, k_insert) unless noted; the caller allocates them. */
typedef struct gc_map_update_out {
  int32_t* insert_indices;       /* the chosen measurement rows: the first k_insert of a stable descending
                                    sort of the tile's score (pipeline.py:1351-1352) */
  uint8_t* insert_valid;         /* valid_new, after the placeholder rule (:1353-1355) */
  int32_t* insert_target_slots;  /* the tile-local eviction slot of each proposal */
  int64_t* new_ids;              /* -1 where not inserted */
  double* prop_Lambdas;          /* (n_active, k_insert, 3, 3) proposals in the world frame (:1373-1375) */
  double* prop_thetas;           /* (n_active, k_insert, 3) */
  double* prop_weights;          /* weights_ins (:1360-1362) */
  double* stats;                 /* (GC_MAP_UPDATE_STATS_HEAD + GC_MAP_UPDATE_STATS_TILE * n_active) */
} gc_map_update_out;

/* Fuse (pipeline.py:1258-1327): rows in blocks of block_size as block_associations_for_fuse
   (primitive_association.py:561-588); every (row, k) whose candidate tile is active, whose
   measurement is valid and whose slot is in range is pushed to the world frame at h_pose6 = z_t
   (:1248-1256) and fused with its responsibility into slot dense tile x m_tile + slot, each slot's
   rows summed in row order. Then every in-range slot number that any candidate of any row names is
   stamped in every active tile (each per-tile fuse receives all of its block's target slots,
   :1302-1324 with primitive_map.py:1112) and every slot of the active tiles gets the fuse's colour
   estimate. Insert plan (:1331-1392): novelty = max(valid / max(sum valid, eps_mass) - row_masses,
   0), score = novelty w - (1 - valid) 1e6, the measurement's tile from its world mean
   (tiling.py:126-145); per active tile the first k_insert rows of a stable descending sort of the
   in-tile scores (others -1e30), valid_new = in_tile & score > -1e20 or all ones when none is, the
   proposals pushed to the world frame and inserted as gc_primitive_map_insert_masked does, tiles in
   the given order on the map the fuse left, global ids running on from next_global_id. Nothing is
   downloaded and the stream is not waited for: the caller reads the outputs after its own download. */
typedef struct {
  double eps_lift;
  double eps_mass;
  double h_tile;
  double recency_decay_lambda;
} gc_map_update_cfg;
int32_t gc_primitive_map_update(gc_ctx* ctx, const gc_primitive_map* map, const gc_map_update_in* in,
                                const double* h_pose6, const gc_map_update_cfg* cfg, double timestamp,
                                int64_t scan_seq, int64_t next_global_id, const gc_map_update_out* out);

/* The maintenance of step 12b (backend/pipeline.py:1412-1447) over all active tiles in one pass:
   per active tile primitive_map_cull (primitive_map.py:1175-1305), primitive_map_forget (:1314-1390)
   and primitive_map_merge_reduce (:1809-2030), with the results of the per-tile entries above run in
   that order on each tile. Tile a is the slot range [dense[a] * m_tile, (dense[a] + 1) * m_tile);
   d_active_dense (device) and h_active_dense (host) hold the same n_active distinct dense tiles, each
   in [0, m_slots / m_tile). max_primitives < 0 = no cap on the survivors.

   What the per-tile entries decide on the host after a download is decided here per tile on the
   device: whether the tile takes the max_primitives branch (one segmented descending sort of
   weight * valid over the active tiles is always launched when max_primitives >= 0), and the
   merge's no-op tests (fewer than 2 valid slots after the cull). Host-known, and launching nothing:
   m_tile < 2 or max_pairs <= 0, and the tile-size cap max_tile_size > 0 && m_tile > max_tile_size.
   Otherwise the merge runs over the tiles in groups of max(1, min(max_sort_keys / P,
   GC_MAP_MAINTAIN_GROUP_TILES)) with P = m_tile (m_tile - 1) / 2 pair keys per tile, one segmented
   stable sort per group, and requires m_tile <= 65536. max_sort_keys = 0 selects
   GC_MAP_MAINTAIN_SORT_KEYS: a group's keys, values and sort buffers take 36 B per key (288 MiB), its
   per-tile buffers (105 B per slot, 2 KiB of digit counts per tile) at most 40 MiB more; the cull's
   sort adds 24 B per active slot when max_primitives >= 0 and shares the group's block. A single tile
   with P > max_sort_keys is sorted whole, as gc_primitive_map_merge_reduce does.

   d_stats (device, caller-allocated, GC_MAP_MAINTAIN_STATS_TILE doubles per active tile): [0] valid
   count before, [1] n_culled, [2] mass_dropped (0 when nothing was culled), [3] sum of the weights
   of all slots before the forget, [4] the cull threshold used, [5] n_merged, [6] valid count after,
   [7] the merge state: GC_MAP_MAINTAIN_MERGE_RAN, _NOOP (m_tile < 2, fewer than 2 valid slots after
   the cull, or max_pairs <= 0: the reference's exact no-op) or _CAPPED (skipped by the tile-size
   cap). Nothing is downloaded and the stream is not waited for; the scratch is sized once before
   the first launch. n_active = 0 succeeds and launches nothing. */
#define GC_MAP_MAINTAIN_STATS_TILE 8
#define GC_MAP_MAINTAIN_MERGE_RAN 0
#define GC_MAP_MAINTAIN_MERGE_NOOP 1
#define GC_MAP_MAINTAIN_MERGE_CAPPED 2
#define GC_MAP_MAINTAIN_SORT_KEYS (1 << 23)
#define GC_MAP_MAINTAIN_GROUP_TILES 4096
typedef struct {
  double primitive_cull_weight_threshold;
  double primitive_forgetting_factor;
  double primitive_merge_threshold;
  double eps_psd;
  double eps_lift;
} gc_map_maintain_cfg;
int32_t gc_primitive_map_maintain(gc_ctx* ctx, const gc_primitive_map* map, int64_t m_tile, int32_t n_active,
                                  const int32_t* d_active_dense, const int32_t* h_active_dense,
                                  const gc_map_maintain_cfg* cfg, int64_t max_primitives, int32_t max_pairs,
                                  int64_t max_tile_size, int64_t max_sort_keys, double* d_stats);

/* primitive_map_recency_inflate (primitive_map.py:1400-1490) over a list of tiles in one pass: what
   gc_primitive_map_recency_inflate does to each tile [dense[a] * m_tile, (dense[a] + 1) * m_tile), with
   no download and no wait. The tile list and its checks are those of gc_primitive_map_maintain
   (d_active_dense on the device and h_active_dense on the host hold the same n_active distinct dense
   tiles, each in [0, m_slots / m_tile)). d_stats (device, caller-allocated, 3 doubles per tile in tile
   order) = [n_valid, sum (1 - decay), sum (1/decay - 1)] over the tile's valid slots, bit for bit what
   the per-tile entry returns for that tile: the same slots per thread, the same block partition and
   the same fixed-order tree, no float atomics. n_active = 0 succeeds and launches nothing. */
int32_t gc_primitive_map_recency_inflate_tiles(gc_ctx* ctx, const gc_primitive_map* map, int64_t m_tile,
                                               int32_t n_active, const int32_t* d_active_dense,
                                               const int32_t* h_active_dense, int64_t scan_seq,
                                               double decay_lambda, double min_scale, double* d_stats);

/* ------------------------------------------------------------------------------------------
 * Tile residency: the reference's AtlasMap creates tiles on demand (primitive_map.py:183-211); the
 * device map holds a fixed number of slabs, and a tile that has to leave its slab is kept by the
 * host as an image. Each entry works on one tile [slot0, slot0 + n_slots), as the maintenance
 * entries do.
 *
 * The image of a tile is n_slots records of gc_primitive_map_record_layout(n_lobes) (n_slots x
 * slot_bytes_out bytes), whatever the map's own layout, so an image exported from a packed map can
 * be imported into a per-field map and back. valid_mask is the low byte of its 8-byte word; padding
 * bytes of an image are not part of its contract. A packed map holding all sixteen fields moves the
 * image with one copy; any other map gathers / scatters it through the context's scratch with one
 * kernel. Fields the map does not hold (no colour tracking, no maintenance fields) are written as
 * create_empty_tile has them (primitive_map.py:148-175: zeros, rgb = 0.5) on export and ignored on
 * import.
 *
 * NONE OF THESE ENTRIES WAITS FOR THE STREAM. The caller waits once (gc_ctx_synchronize) after the
 * last entry of its plan, and h_image must stay allocated, and for an import unchanged, until then.
 * ------------------------------------------------------------------------------------------ */
int32_t gc_primitive_map_tile_export(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                                     void* h_image);
int32_t gc_primitive_map_tile_import(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots,
                                     const void* h_image);
/* Every slot of the tile becomes create_empty_tile's (primitive_map.py:148-175): zeros in every field
   the map holds, rgb = 0.5. One kernel. The caller marks the tile's colours not current
   (gc_primitive_map.colors_current), as for a new map. */
int32_t gc_primitive_map_tile_reset(gc_ctx* ctx, const gc_primitive_map* map, int64_t slot0, int64_t n_slots);

/* ------------------------------------------------------------------------------------------
 * Map view + OT association (the current PrimitiveMap pose-evidence path).
 * ------------------------------------------------------------------------------------------ */
/* AtlasMapView (primitive_map.py:236-300) in device memory: V = n_tiles * m_tile_view entries,
   tile-major. The caller allocates every array; tile_ids is a device copy of the view tile ids. */
typedef struct gc_map_view {
  int32_t n_tiles;
  int32_t m_tile_view;
  int32_t n_lobes;
  int32_t pad_;
  int64_t* tile_ids;                /* (T) packed MA-hex tile ids */
  int64_t* candidate_tile_ids;      /* (V) */
  int64_t* candidate_slots;         /* (V) tile-local slot */
  uint8_t* valid_mask;              /* (V) */
  double* positions;                /* (V, 3) solve(Λ + εI, θ) */
  double* covariances;              /* (V, 3, 3) inv(Λ + εI) */
  double* directions;               /* (V, 3) η_sum / (‖η_sum‖ + ε_mass) */
  double* kappas;                   /* (V) ‖η_sum‖ */
  double* weights;                  /* (V) */
  int64_t* primitive_ids;           /* (V) */
  int64_t* last_supported_scan_seq; /* (V) */
  double* etas;                     /* (V, n_lobes, 3) */
  double* colors;                   /* (V, 3) rgb (0.5 where the map has no colour fields) */
} gc_map_view;

/* extract_atlas_map_view (primitive_map.py:356-451): for view tile t, the top m_tile_view slots of
   dense map tile h_dense_tiles[t] (slot range [d * m_tile, (d+1) * m_tile); -1 = missing, an empty
   tile) by weight, invalid slots last, ties by slot (_select_topk_slots_fixed :304-322). */
int32_t gc_extract_map_view(gc_ctx* ctx, const gc_primitive_map* map, int64_t m_tile, const int64_t* h_dense_tiles,
                            const int64_t* h_tile_ids, double eps_lift, double eps_mass, const gc_map_view* view);

/* AssociationConfig (primitive_association.py:205-236) and the call's eps_lift */
typedef struct {
  double k_assoc;
  double k_sinkhorn;
  double beta;
  double epsilon;
  double tau_a;
  double tau_b;
  double cost_subtract_row_min; /* 0 or 1 */
  double weight_proportional;   /* 1: a_policy WEIGHT_PROPORTIONAL, 0: UNIFORM */
  double eps_mass;
  double h_tile;
  double r_stencil_tiles_xy;
  double r_stencil_tiles_z;
  double scan_seq;
  double recency_decay_lambda;
  double eps_lift;
} gc_ot_cfg;
#define GC_OT_CERT_LEN 13 /* [marginal_defect_a, marginal_defect_b, transport_mass_total, sum_a, sum_b, sum_m,
                             sum_novel, ess_ot, nonzero_a, nonzero_b, total_cost, n_valid_meas, n_valid_map] */
/* associate_primitives_ot (operators/primitive_association.py:239-553): N measurement primitives
   (info form + vMF lobes) against a map view. Outputs (device, caller-allocated, K = k_assoc <= 16):
   responsibilities (N, K), candidate pool indices int32 (N, K), candidate tile ids / slots int64
   (N, K), row masses (N), cost matrix (N, K). h_cert_out (host) = GC_OT_CERT_LEN values; with no
   valid measurement or map entry every output is zero and n_valid_* tell which. */
int32_t gc_associate_primitives_ot(gc_ctx* ctx, int64_t N, int32_t n_lobes, const double* d_Lambdas,
                                   const double* d_thetas, const double* d_etas, const double* d_weights,
                                   const uint8_t* d_valid, const gc_map_view* view, const gc_ot_cfg* cfg,
                                   double* d_resp_out, int32_t* d_cand_out, int64_t* d_cand_tile_out,
                                   int64_t* d_cand_slot_out, double* d_row_mass_out, double* d_cost_out,
                                   double* h_cert_out);

/* The candidate statistics of the map branch (backend/pipeline.py:879-905) from an association's pool
   indices int32 (N, K) and candidate tile ids int64 (N, K), the measurement rows' valid mask (N) and
   the view the indices point into (clamped into it, as a JAX gather does). Per row: cand_valid =
   view.valid_mask[pool index], the number of valid candidates, and the number of distinct tile ids
   among them. d_out3 (device) = [candidate_tiles_per_meas_mean, candidate_primitives_per_meas_mean,
   candidate_primitives_per_meas_p95]: the two sums over valid rows divided by max(sum valid,
   eps_mass), and entry min(int(0.95 N), N - 1) of the ascending sort of the counts with -1 at invalid
   rows, taken from a histogram of the K + 2 possible values. Integer sums: exact and order-free. No
   valid row (or N = 0): all three are 0. 1 <= K <= 16. Nothing is downloaded, no wait. */
int32_t gc_association_candidate_stats(gc_ctx* ctx, int64_t N, int32_t K, const uint8_t* d_valid_meas,
                                       const int32_t* d_cand_pool, const int64_t* d_cand_tile,
                                       const gc_map_view* view, double eps_mass, double* d_out3);

#define GC_VPE_PARTS 26  /* per hypothesis: L_trans(9) h_trans(3) L_rot(9) h_rot(3) cost_trans cost_rot */
#define GC_VPE_CERT 4    /* host: [n_valid_meas, n_valid_map, sum_row_masses, mean_row_mass] */
/* visual_pose_evidence (operators/visual_pose_evidence.py:261-436; translation WLS :74-162, vMF
   scatter rotation :165-253), batched over H linearisation poses that share one association.
   N measurement primitives (info form + vMF lobes, as gc_associate_primitives_ot takes them), the
   association's responsibilities (N, K), pool indices int32 (N, K; clamped into the view, as a JAX
   gather does) and row masses (N), and the view they index. d_pose6 (H, 6) = [t, rotvec] per
   hypothesis. Outputs (device, caller-allocated): L_pose (H, 22, 22) = eps_lift I with L_trans at
   [0:3, 0:3] and L_rot at [3:6, 3:6], h_pose (H, 22) laid out the same way, parts (H, GC_VPE_PARTS).
   h_cert (host) = GC_VPE_CERT values. With no valid measurement or no valid view entry every
   hypothesis gets L_pose = eps_lift I, h_pose = 0 and parts = 0 (the reference's empty branch,
   :297-318). H = 0 fills h_cert only (the pose and output pointers may then be NULL); N = 0 is the
   empty branch. Sums run in a fixed order: results are bitwise reproducible, and row h of a batch
   equals the H = 1 call with pose h. GC_ERR_ARG for N < 0, K outside [1, 16], n_lobes outside
   [1, 8], H < 0 or NULL pointers. */
int32_t gc_visual_pose_evidence(gc_ctx* ctx, int64_t N, int32_t K, int32_t n_lobes, const double* d_Lambdas,
                                const double* d_thetas, const double* d_etas, const uint8_t* d_valid,
                                const double* d_resp, const int32_t* d_pool_idx, const double* d_row_masses,
                                const gc_map_view* view, int32_t H, const double* d_pose6, double eps_lift,
                                double eps_mass, double* d_L_pose, double* d_h_pose, double* d_parts,
                                double* h_cert);

/* SurfelExtractionConfig (operators/lidar_surfel_extraction.py:43-62), then the lobes per row (GC_VMF_N_LOBES) */
typedef struct {
  double n_surfel;
  double n_feat;
  double voxel_size_m;
  double hex3d_num_cells_1;
  double hex3d_num_cells_2;
  double hex3d_num_cells_z;
  double hex3d_max_occupants;
  double min_points_per_voxel;
  double sensor_noise_var_per_axis;
  double wishart_nu;
  double wishart_psi_scale;
  double kappa_main_scale;
  double kappa_min;
  double kappa_max;
  double eig_min;
  double eps_lift;
  double n_lobes;
} gc_surfel_cfg;
#define GC_SURFEL_MAX_POINTS (1 << 22)  /* N */
#define GC_SURFEL_MAX_CELLS 16384       /* each grid size, and the cells in all: cell keys are below 2^14 */
#define GC_SURFEL_MAX_OCCUPANTS 1024    /* hex3d_max_occupants: bucket slots per cell */
/* extract_lidar_surfels (operators/lidar_surfel_extraction.py:219-431; MA-hex hash grid
   common/ma_hex_web.py:221-303; batch rows structures/measurement_batch.py:262-347): the LiDAR
   slice of a MeasurementBatch from the N deskewed points (N, 3), timestamps (N) and weights (N) of
   one scan (device); cfg (host) is gc_surfel_cfg.
   Outputs (device, caller-allocated, n_total = n_feat + n_surfel rows): Lambdas (n_total, 3, 3),
   thetas (n_total, 3), etas (n_total, n_lobes, 3), weights (n_total), sources int32 (n_total),
   source_indices int32 (n_total), valid_mask uint8 (n_total), timestamps (n_total), colors
   (n_total, 3). Only rows n_feat + j, j < n_valid, are written: the caller fills the arrays with the
   base batch (or zeros) first, and the camera slice and the tail of the LiDAR slice keep it.
   d_slot_cells (int32, n_surfel; may be NULL) receives the hash cell each slot came from, -1 past
   n_valid. h_n_valid (host) = min(valid cells, n_surfel); the call waits for it (the reference's one
   sync, :206). Points with a coordinate at or beyond 0.1 x 1e6 (the parser's non-finite sentinel) or
   NaN take no part. Valid cells are taken in ascending cell id; a cell keeps its first
   max_occupants points in ascending point index; all sums run in a fixed order, so the batch is
   bitwise reproducible. GC_ERR_ARG for N outside [0, 2^22], a grid size outside [1, 16384] or more
   than 16384 cells in all, max_occupants outside [1, 1024], n_surfel < 1, voxel_size_m <= 0 or
   2e5 / voxel_size_m >= 2^31, n_lobes outside [1, 8], or NULL pointers. */
int32_t gc_extract_lidar_surfels(gc_ctx* ctx, int64_t N, const double* d_points, const double* d_timestamps,
                                 const double* d_weights, const gc_surfel_cfg* cfg, double* d_Lambdas, double* d_thetas,
                                 double* d_etas, double* d_weights_out, int32_t* d_sources,
                                 int32_t* d_source_indices, uint8_t* d_valid_mask, double* d_timestamps_out,
                                 double* d_colors, int32_t* d_slot_cells, int32_t* h_n_valid);

/* RGB-D surfel extraction (this build's; the reference's camera path is ORB-only; DESIGN.md §4, "Depth
   surfels"): coloured rows of the camera slice (sources = 0) of a MeasurementBatch, in the base frame,
   from one depth image d_depth (H, W; float32, metres; device) and its rgb image d_rgb8 (H, W, 3; uint8;
   device; may be NULL). h_intrinsics (host) = [fx, fy, cx, cy]; h_R_base_camera (9, row-major) and
   h_t_base_camera (3) on the host; n_camera_valid_in the camera rows already used. cfg (host) is
   gc_surfel_cfg, read for n_feat, n_surfel, wishart_*, kappa_*, eig_min, eps_lift and n_lobes; its hash-grid
   members, min_points_per_voxel and sensor_noise_var_per_axis are ignored.
   Cells: cell_px x cell_px pixel blocks in row-major order, n_cx = ceil(W / cell_px), cell id = cy n_cx +
   cx; H and W need not be multiples, and the pixels of an edge cell outside the image are missing. A pixel
   is used where its depth z is finite and min_depth < z < max_depth (strict). Pixel (row i, column j)
   backprojects through its centre, p_c = z ((j + 0.5 - cx) / fx, (i + 0.5 - cy) / fy, 1) (the camera
   renderer's convention, not the integer keypoints of gc_camera_features_lift), and
   p_b = R_base_camera p_c + t_base_camera. Per cell over the used pixels, unit weights: n, mean = sum p / n,
   C = sum (p - mean)(p - mean)^T / n (two passes), zbar the mean of z, and the integer sums of R, G, B.
   The plane fit and the row are gc_extract_lidar_surfels' from `cov = C + eig_min I` on (the eigenvector of
   the smallest eigenvalue as the normal, n_z >= 0 in the base frame, the in-plane basis, the Wishart
   regularisation, kappa, the information form with eps_lift), with w_sum = n and, in the place of
   sensor_noise_var_per_axis, sigma_z(zbar)^2: sigma_z = sigma0 + slope zbar (depth_model 0) or
   sigma0 + slope zbar^2 (1). A cell is valid iff n >= max(3, ceil(min_fill cell_px^2)),
   lambda_min(C) <= (plane_gate sigma_z(zbar))^2 (lambda_min(C) as the fit's smallest eigenvalue less eig_min)
   and |n . (mean - t_base_camera)| / |mean - t_base_camera| >= min_cos_incidence.
   Row: weights = weight_scale n / cell_px^2, timestamps = timestamp_sec, sources = 0, colors = (sum R,
   sum G, sum B) / (255 n) or, with d_rgb8 NULL, the LiDAR rows' grey 0.25 + 0.25 (n_z + 1); lobes 1.. of
   etas zero, valid_mask 1. Selection: free = n_feat - n_camera_valid_in, V the valid cells in ascending
   cell id; V <= free keeps all, otherwise the cell of rank r is kept iff floor((r + 1) free / V) >
   floor(r free / V), which keeps exactly `free` cells spread evenly over the image. The kept cell of
   kept-rank k goes to row n_camera_valid_in + k with source_indices = row.
   Outputs (device, caller-allocated and caller-filled, as gc_extract_lidar_surfels lays them out): only the
   kept rows of the nine arrays are written. d_slot_cells (int32, n_feat) receives the cell id of every row
   written and -1 for every other row of [0, n_feat). h_n_valid (host) = the kept count; the call waits for
   it. With free = 0 or no valid cell only d_slot_cells is written. All sums run in a fixed order: the
   batch is bitwise reproducible. GC_ERR_ARG before any launch for H or W outside [1, 16384], H W >
   GC_IMAGE_MAX_PIXELS, cell_px outside [4, 32], more than GC_SURFEL_MAX_CELLS cells, n_camera_valid_in
   outside [0, n_feat], min_fill outside (0, 1], min_depth < 0 or min_depth >= max_depth, depth_model not 0
   or 1, sigma0 <= 0, slope < 0, plane_gate <= 0, min_cos_incidence outside [0, 1), n_lobes outside [1, 8],
   fx or fy = 0, a non-finite parameter, intrinsic, R or t, or NULL pointers. */
int32_t gc_extract_depth_surfels(gc_ctx* ctx, const float* d_depth, const uint8_t* d_rgb8, int32_t H, int32_t W,
                                 const double* h_intrinsics, const double* h_R_base_camera, const double* h_t_base_camera,
                                 double timestamp_sec, int32_t n_camera_valid_in, const gc_surfel_cfg* cfg, int32_t cell_px,
                                 double min_fill, double min_depth, double max_depth, int32_t depth_model, double sigma0,
                                 double slope, double plane_gate, double min_cos_incidence, double weight_scale,
                                 double* d_Lambdas, double* d_thetas, double* d_etas, double* d_weights_out,
                                 int32_t* d_sources, int32_t* d_source_indices, uint8_t* d_valid_mask,
                                 double* d_timestamps_out, double* d_colors, int32_t* d_slot_cells, int32_t* h_n_valid);

/* LidarCameraDepthFusionConfig in field order (frontend/sensors/lidar_camera_depth_fusion.py:29-63) */
typedef struct {
  double depth_fusion_weight_camera;
  double depth_fusion_weight_lidar;
  double gamma_lidar;
  double lidar_projection_radius_pix;
  double lidar_plane_fit_min_points;
  double lidar_depth_base_sigma_m;
  double lidar_incidence_sigma_scale; /* the reference never reads it */
  double depth_var_min_m2;
  double point_support_n0;
  double point_support_alpha;
  double spread_mad_beta;
  double repr_gamma;
  double lidar_ray_plane_fit_max_points;
  double plane_intersection_delta;
  double plane_angle_sigmoid_alpha;
  double plane_angle_sigmoid_t;
  double plane_planarity_sigmoid_beta;
  double plane_planarity_rho0;
  double plane_residual_exp_gamma;
  double plane_fit_eps;
  double depth_min_m;
  double depth_sigma_max_sq;
  double depth_min_sigmoid_alpha_z;
} gc_cam_cfg;
#define GC_CAM_EV 9          /* per query: Lambda_A theta_A Lambda_B theta_B Lambda_ell theta_ell, then Route
                                B's z*, sigma^2 and w (NaN, NaN, 0 where Route B does not run) */
#define GC_CAM_MAX_NEAR 1024 /* in-radius LiDAR points one query can hold */
#define GC_CAM_MAX_POINTS (1 << 22)  /* N */
#define GC_CAM_MAX_QUERIES 4096      /* rows of one camera batch: the query pixels M here, the keypoints of
                                        gc_camera_features_lift and nfeatures of gc_keypoints_detect */
#define GC_CAM_MAX_FIT_POINTS 256    /* lidar_ray_plane_fit_max_points: one fitted point per thread */
/* lidar_depth_evidence (frontend/sensors/lidar_camera_depth_fusion.py:389-442; _project_camera :80-96,
   Route A :99-164, Route B :242-386, _fit_plane_weighted :207-239): the LiDAR depth evidence of M
   query pixels d_uv (M, 2) from N points in the camera frame (N, 3). h_intrinsics (host) = [fx, fy,
   cx, cy]; cfg (host) is gc_cam_cfg; d_point_weights (N; may be NULL: uniform) weighs
   Route B's plane fit. Outputs (device, caller-allocated): d_evidence (M, GC_CAM_EV) and d_counts
   int32 (M), the number of z > 0 points whose projection lies within the radius of the query. The
   candidates of a query are taken in ascending point index, the k_use nearest the ray by (distance,
   index), and every sum runs in a fixed order: the outputs are bitwise reproducible. The call waits
   once, for the candidate-cap word. GC_ERR_ARG for N outside [0, 2^22], M outside [0, 4096], a
   radius <= 0, lidar_plane_fit_min_points < 1, lidar_ray_plane_fit_max_points outside [1, 256],
   non-finite intrinsics or fx, fy = 0, NULL pointers, or a query with more than GC_CAM_MAX_NEAR
   points within its radius (the outputs are then not to be used; the reference has no such cap). */
int32_t gc_lidar_depth_evidence(gc_ctx* ctx, int64_t N, const double* d_points_cam, int64_t M, const double* d_uv,
                                const double* h_intrinsics, const gc_cam_cfg* cfg, const double* d_point_weights,
                                double* d_evidence, int32_t* d_counts);

/* The camera half of a scan's MeasurementBatch in one call (backend/backend_node.py:1872-1925):
   the N base-frame points go to the camera frame (p_cam = R^T (p - t), h_R9 row-major and h_t3 on the
   host; both NULL: the points are in the camera frame already and rows stay there), lidar_depth_evidence
   runs for the M features' pixels d_uv (M, 2), splat_prep_fused (frontend/sensors/splat_prep.py:37-134)
   fuses it with each feature's camera depth (d_Lambda_c, d_theta_c (M)) or falls back to the
   feature's own d_xyz (M, 3) and d_cov_xyz (M, 3, 3), every feature goes to the base frame, and
   feature_list_to_camera_batch (backend/camera_batch_utils.py:23-86) with
   measurement_batch_from_camera_splats (backend/structures/measurement_batch.py:165-259) writes rows
   [0, min(M, n_feat)). d_mu_app (M, 3) is read where d_has_mu_app (uint8, M) is set (else the
   direction is the row's position), d_color (M, 3) where d_has_color is set (else grey 0.5).
   Outputs (device, caller-allocated): the nine batch arrays of n_total = n_feat + n_surfel rows as
   gc_extract_lidar_surfels lays them out, every row from min(M, n_feat) on zero; d_fused_xyz
   (M, 3), d_fused_cov (M, 3, 3) (camera frame, as splat_prep_fused returns them) and d_fused_flag
   (uint8, M; 0 = fell back); d_evidence and d_counts as above. One wait, for the candidate-cap word.
   GC_ERR_ARG as gc_lidar_depth_evidence, and for n_feat or n_surfel outside [0, 2^24] or n_lobes
   outside [1, 8]. */
int32_t gc_camera_measurement_batch(gc_ctx* ctx, int64_t N, const double* d_points_base, const double* h_R9,
                                    const double* h_t3, int64_t M, const double* d_uv, const double* d_Lambda_c,
                                    const double* d_theta_c, const double* d_weight, const double* d_kappa,
                                    const double* d_mu_app, const uint8_t* d_has_mu_app, const double* d_color,
                                    const uint8_t* d_has_color, const double* d_xyz, const double* d_cov_xyz,
                                    const double* h_intrinsics, const gc_cam_cfg* cfg, double pixel_sigma,
                                    double timestamp_sec, int32_t n_feat, int32_t n_surfel, int32_t n_lobes,
                                    double eps_lift, double* d_Lambdas, double* d_thetas, double* d_etas,
                                    double* d_weights_out, int32_t* d_sources, int32_t* d_source_indices,
                                    uint8_t* d_valid_mask, double* d_timestamps_out, double* d_colors,
                                    double* d_fused_xyz, double* d_fused_cov, uint8_t* d_fused_flag,
                                    double* d_evidence, int32_t* d_counts);

/* The visual feature node's parameters in the order it declares them (src/visual_feature_node.cpp:74-101) */
typedef struct {
  double depth_sample_mode; /* 0 nearest, 1 median3, 2 median5, 3 hex */
  double pixel_sigma;
  double depth_model;       /* 0 linear, 1 quadratic */
  double depth_sigma0;
  double depth_sigma_slope;
  double min_depth_m;
  double max_depth_m;
  double depth_validity_slope;
  double response_soft_scale;
  double depth_scale;
  double cov_reg_eps;       /* declared by the node and never read */
  double invalid_cov_inflate;
  double hex_radius;
  double quad_fit_radius;
  double quad_fit_min_points;
  double quad_fit_lstsq_eps;
  double student_t_nu;
  double student_t_w_min;
  double ma_tau;
  double ma_delta_inflate;
  double kappa0;
  double kappa_alpha;
  double kappa_max;
  double kappa_min;
} gc_camfeat_cfg;
#define GC_CAMFEAT_AUX 6      /* per keypoint: depth_sigma_c_sq (NaN without a valid depth), z_m (NaN
                                 without), the depth window's valid count, the quadratic fit's point
                                 count (0 without a valid depth), lam_min and K (0 without a fit) */
#define GC_CAMFEAT_MAX_RADIUS 3       /* max(1, hex_radius), max(1, quad_fit_radius): one lane per window pixel */
#define GC_IMAGE_MAX_PIXELS (1 << 26) /* H W of an image, here and in the keypoint detector (and each axis of
                                         gc_keypoints_resize_table) */
/* The image side of the camera features (src/visual_feature_node.cpp:493-652 without ORB, and what
   _feature_batch_to_list makes of the message, backend/backend_node.py:1589-1645): M keypoints d_kp
   (M, 3) = (u, v, response) in f64, the depth image d_depth (float32, H x W, row-major, metres before
   depth_scale) and the colour image d_rgb (uint8, H x W x 3; NULL: no colours, d_color 0 and
   d_has_color 0) -> per keypoint depth_sample (:228-297; std::round, the window clipped to the image,
   the element of rank size/2, the variance from 4 values up) or depth_sample_hex (:299-348),
   student_t_effective_var (:350-369), depth_weight, response_weight and depth_sigma (:196-226),
   quadratic_fit (:401-491: the window about the rounded pixel, coordinates relative to the keypoint,
   normal equations with the ridge quad_fit_lstsq_eps solved by an unpivoted LDL^T), backproject and
   backprojection_cov (:371-399) and the assembly (:547-634). h_intrinsics (host) = [fx, fy, cx, cy];
   cfg (host) is gc_camfeat_cfg. Outputs (device, caller-allocated), laid out as
   gc_camera_measurement_batch reads its feature arguments: d_uv (M, 2), d_Lambda_c, d_theta_c,
   d_weight, d_kappa (M), d_mu_app (M, 3; the normal over (norm + 1e-12), 0 without a fit),
   d_has_mu_app (uint8; the rows with a fit), d_color (M, 3), d_has_color (uint8), d_xyz (M, 3),
   d_cov_xyz (M, 3, 3; a non-finite covariance is replaced by 1e6 I, :1600-1601) and d_aux
   (M, GC_CAMFEAT_AUX). A keypoint without a valid depth gets xyz 0, invalid_cov_inflate I, weight 0
   and Lambda_c = theta_c = 0. One wavefront per keypoint, every sum in a fixed order, no atomics: the
   outputs are bitwise reproducible. No wait. GC_ERR_ARG for M outside [0, 4096], H or W < 1 or
   H W > 2^26, max(1, hex_radius) or max(1, quad_fit_radius) outside [1, 3], quad_fit_min_points < 1,
   an unknown mode or model code, non-finite intrinsics or fx, fy = 0, NaN in cfg, or NULL pointers
   (d_rgb excepted). */
int32_t gc_camera_features_lift(gc_ctx* ctx, int32_t H, int32_t W, const float* d_depth, const uint8_t* d_rgb,
                                int64_t M, const double* d_kp, const double* h_intrinsics, const gc_camfeat_cfg* cfg,
                                double* d_uv, double* d_Lambda_c, double* d_theta_c, double* d_weight,
                                double* d_kappa, double* d_mu_app, uint8_t* d_has_mu_app, double* d_color,
                                uint8_t* d_has_color, double* d_xyz, double* d_cov_xyz, double* d_aux);

/* The arguments of the node's cv::ORB::create (src/visual_feature_node.cpp:149-158; 512, 1.2, 8, 31, 20) and
   Harris's k (0.04) */
typedef struct {
  double nfeatures;
  double scale_factor;
  double nlevels;
  double edge_threshold;
  double fast_threshold;
  double harris_k;
} gc_kp_cfg;
#define GC_KP_MAX_LEVELS 16
#define GC_KP_PLAN_ROW 5    /* per level: W_l, H_l, the quota n_l, the candidate capacity
                               ceil(W_l / 2) ceil(H_l / 2), the level's byte offset in the pyramid */
#define GC_KP_COUNTS_LEN 49 /* per level l < GC_KP_MAX_LEVELS [3 l .. 3 l + 2]: the corners after non-maximum
                               suppression, after the border, and kept; [48]: the total */
/* The plan of the keypoint detector for an H x W image (host only; build-defined, DESIGN.md §4 "Keypoint
   detector"; the detector half of the node's ORB, src/visual_feature_node.cpp:149-158, :512-535):
   s_l = (double)(float)pow((double)(float)scale_factor, l), W_l = rint(W / s_l) and H_l = rint(H / s_l)
   (halves to even, at least 1), the quotas n_l of ORB's geometric split (the last level takes what is
   left), the candidate capacities and the levels' byte offsets in the pyramid (each level row-major
   uint8 on a 256-byte boundary). h_levels (GC_KP_MAX_LEVELS, GC_KP_PLAN_ROW) and h_scales
   (GC_KP_MAX_LEVELS), zero from nlevels on; h_bytes = [pyramid bytes, workspace bytes (the context's
   scratch a call carves)]. GC_ERR_ARG as gc_keypoints_detect. */
int32_t gc_keypoints_plan(int32_t H, int32_t W, const gc_kp_cfg* cfg, int64_t* h_levels, double* h_scales,
                          int64_t* h_bytes);

/* Test entry (host only), in the manner of gc_test_bounded_wait: the index and weight table of one axis
   of the detector's 8-bit bilinear resize n_src -> n_dst (build-defined; src/visual_feature_node.cpp:149-158,
   :512-535 run cv::ORB's pyramid): per destination j, f = (j + 0.5) n_src / n_dst - 0.5, h_i0 = floor(f),
   h_w1 = rint((f - h_i0) 2048), clamped to the source ((0, 0) below, (n_src - 1, 0) from the last sample
   on). GC_ERR_ARG for a size outside [1, 2^26] or NULL pointers. */
int32_t gc_keypoints_resize_table(int64_t n_src, int64_t n_dst, int32_t* h_i0, int32_t* h_w1);

/* The detector half of the node's ORB (src/visual_feature_node.cpp:149-158, :512-535; cv::ORB with
   HARRIS_SCORE) on the device, build-defined: it follows the published algorithms and DESIGN.md §4
   "Keypoint detector" states every step; it was not checked against OpenCV and does not claim its bits.
   d_image (device, uint8, H x W x channels; channels 3: rgb8, 1: grey) -> grey (4899 R + 9617 G +
   1868 B + 8192) >> 14 -> nlevels pyramid levels in d_pyramid (gc_keypoints_plan's bytes and offsets;
   8-bit bilinear, 11-bit weights) -> per level FAST-9/16 with score max-min-arc - 1, strict 3 x 3
   non-maximum suppression, the border edge_threshold, the 2 n_l best by (score descending, raster index
   ascending), their 7 x 7 Harris responses in f64, the n_l best by (response descending, raster index
   ascending). Outputs (device, caller-allocated): d_kp (nfeatures, 3) = (x s_l, y s_l, response) f64,
   levels ascending; d_meta (nfeatures, 4) int32 = (level, x, y, FAST score); d_counts
   (GC_KP_COUNTS_LEN int32). Rows from the total on are zero. No angle, size, descriptor or blur.
   Integer arithmetic and seven f64 operations per response: bitwise reproducible and independent of
   the order the candidates are found in. No wait: the resize tables go up in one staged upload while
   they fit 512 KiB (33 KB at 640 x 480), else per level, and only a level whose own tables exceed
   512 KiB waits for its upload. GC_ERR_ARG before any launch for H or W < 1 or H W > 2^26, channels not 1 or 3,
   nfeatures outside [1, 4096], nlevels outside [1, 16], a scale_factor not finite or <= 1 as float32,
   fast_threshold outside [1, 254], edge_threshold outside [4, 1024] (4 keeps the Harris reads inside
   the image), a non-finite harris_k, a non-integer count, or NULL pointers. */
int32_t gc_keypoints_detect(gc_ctx* ctx, int32_t H, int32_t W, int32_t channels, const uint8_t* d_image,
                            const gc_kp_cfg* cfg, uint8_t* d_pyramid, double* d_kp, int32_t* d_meta,
                            int32_t* d_counts);

/* measurement_batch_from_camera_splats (backend/structures/measurement_batch.py:165-259): rows
   [0, min(N, n_feat)) of a fresh batch from positions (N, 3), covariances (N, 3, 3), directions
   (N, 3), kappas, weights, timestamps (N) and colours (N, 3; may be NULL: grey 0.5), all on the
   device: Lambda = inv(Sigma + eps_lift I), theta = Lambda mu, eta lobe 0 = kappa d, colours clipped
   to [0, 1], sources 0, source_indices = row, valid_mask 1; every other row zero. No wait.
   GC_ERR_ARG for N outside [0, 2^24], budgets as above, or NULL pointers. */
int32_t gc_measurement_batch_from_camera_splats(gc_ctx* ctx, int64_t N, const double* d_positions,
                                                const double* d_covariances, const double* d_directions,
                                                const double* d_kappas, const double* d_weights,
                                                const double* d_timestamps, const double* d_colors_in,
                                                int32_t n_feat, int32_t n_surfel, int32_t n_lobes, double eps_lift,
                                                double* d_Lambdas, double* d_thetas, double* d_etas,
                                                double* d_weights_out, int32_t* d_sources,
                                                int32_t* d_source_indices, uint8_t* d_valid_mask,
                                                double* d_timestamps_out, double* d_colors);

/* ------------------------------------------------------------------------------------------
 * Rendering the map: the renderable batch, BEV splat preparation and the EWA tile raster
 * (backend/map_publisher.py, common/bev_pushforward.py, backend/rendering.py).
 * ------------------------------------------------------------------------------------------ */
/* RenderablePrimitiveBatch (backend/structures/primitive_map.py:454-471) in device memory, plus the
   recency it was ordered by. The caller allocates every array for the view's V entries. */
typedef struct gc_render_batch {
  int32_t n_lobes;
  int32_t pad_;
  double* mu_world;                 /* (V, 3) */
  double* Sigma_world;              /* (V, 3, 3) */
  double* Lambda_world;             /* (V, 3, 3) inv(Sigma_world + eps_lift I) */
  double* eta;                      /* (V, n_lobes, 3) */
  double* mass;                     /* (V) */
  double* color;                    /* (V, 3) the view's colors (the map's rgb) */
  int64_t* primitive_ids;           /* (V) */
  int64_t* last_supported_scan_seq; /* (V) */
} gc_render_batch;

/* PrimitiveMapPublisher.publish (backend/map_publisher.py:143-242) from a map view: the entries with
   valid_mask, in the order np.lexsort((primitive_ids, -last_supported_scan_seq)) (:200: newest first,
   ties by ascending primitive id), compacted into rows [0, count); every row from count on is zero.
   Lambda_world = inv(Sigma_world + eps_lift I) (:232-233). h_count (host) receives count: the one
   wait. Primitive ids and sequence numbers must be below 2^53 in magnitude (they are sorted as double
   keys). An empty view (V = 0, or no valid entry) gives count = 0; V = 0 launches nothing.
   GC_ERR_ARG for n_lobes outside [1, 8] or unequal in view and batch, V >= 2^31 or NULL pointers. */
int32_t gc_renderable_batch_from_view(gc_ctx* ctx, const gc_map_view* view, double eps_lift, const gc_render_batch* out,
                                      int64_t* h_count);

/* The viewport, SplatRenderingConfig (rendering.py:28-44) and render_tile_ewa's fbm arguments (:307-310) */
typedef struct {
  double origin_x;
  double origin_y;
  double px_per_m;
  double eps;
  double opacity_gamma;
  double logdet0;
  double alpha_min;
  double fbm_octaves;
  double fbm_gain;
  double fbm_seed;
  double fbm_modulate_scale;
} gc_bev_cfg;
/* The 2D splats of n_views views of n primitives, view-major. The caller allocates every array. */
typedef struct gc_bev_splats {
  double* means_px;   /* (n_views, n, 2) column, row */
  double* Sigmas_inv; /* (n_views, n, 2, 2) */
  double* alphas;     /* (n_views, n) */
  double* colors;     /* (n_views, n, 3) */
  double* fbm;        /* (n) */
  double* Sigmas_bev; /* (n_views, n, 2, 2) P Sigma P^T itself; may be NULL */
} gc_bev_splats;

/* The renderers' limits, BEV and camera view alike. */
#define GC_RENDER_MAX_VIEWS 32 /* n_views: the views travel by value as one kernel argument */
#define GC_RENDER_MAX_CAP 256  /* cap: splat records one tile holds in LDS */
#define GC_RENDER_MAX_TILE 32  /* tile_size (rendering.py:267, :320 clamp it to [1, 32]) */
/* Rows [0, n) of a batch as 2D splats, per view v with h_P[v] (2, 3) and h_view_dirs[v] (3) (host):
   mu_bev = P mu, Sigma_bev = (P Sigma) P^T (pushforward_gaussian_3d_to_2d, bev_pushforward.py:59-64);
   means_px = (mu_bev - origin_xy) px_per_m; Sigmas_inv = the closed-form inverse of
   px_per_m^2 Sigma_bev + eps I; alphas = opacity_from_logdet(log det Sigma_bev) (rendering.py:236-244);
   colors = color * vmf_shading_multi_lobe(view_dir, eta, |eta|) * ((1 - s_f) + s_f fbm) with uniform
   lobe weights and no intensity (:117-159, :333-340); fbm = fbm_value_noise at the primitive's world
   (x, y) (:167-209). The integer hash of the noise is the reference's while
   |coordinate| * 2^(octaves - 1) < 2^31. No wait. GC_ERR_ARG for n outside [0, 2^24], n_views outside
   [1, 32], n_lobes outside [1, 8], px_per_m <= 0, fbm_octaves not an integer in [0, 32], fbm_seed not
   an integer in [0, 2^31), a non-finite host value or NULL pointers. */
int32_t gc_bev_splat_prep(gc_ctx* ctx, const gc_render_batch* batch, int64_t n, int32_t n_views, const double* h_P,
                          const double* h_view_dirs, const gc_bev_cfg* cfg, const gc_bev_splats* out);

/* splat_indices_for_tile (rendering.py:252-289) for every tile of every view, then render_tile_ewa
   (:297-355) over each tile's list. Tiles are row-major, T = (H / tile_size) (W / tile_size) per view;
   tile (ty, tx) has origin (ty tile_size, tx tile_size). A splat is kept where none of the four bbox
   comparisons with r = 2 / sqrt(max(lambda_min(Sigma_inv), eps)) rejects it; the kept ones are ordered
   by dist_sq to the tile centre, ties by splat index, and the first cap are taken: d_tile_counts
   (n_views, T) and d_tile_indices (n_views, T, cap), -1 past the count. d_images (n_views, H, W, 3):
   per pixel centre (column + 0.5, row + 0.5) the sums of w_i c_i and w_i with
   w_i = alpha_i exp(clip(-q_i / 2, -log_clip, 0)), in list order, divided by (sum w + 1e-12) where that
   exceeds 1e-12 and clipped to [0, 1]. Bitwise reproducible. No wait. n = 0: zero images and counts,
   no kernel. GC_ERR_ARG for tile_size outside [1, 32], H or W not a multiple of tile_size in
   [1, 16384], cap outside [1, 256], n < 0, n_views outside [1, 32], n_views * T * n >= 2^32 or NULL
   pointers. */
int32_t gc_render_ewa_tiles(gc_ctx* ctx, int32_t n_views, int64_t n, const gc_bev_splats* splats, int32_t H, int32_t W,
                            int32_t tile_size, int32_t cap, double log_clip, double eps, double* d_images,
                            int32_t* d_tile_counts, int32_t* d_tile_indices);

/* splat_indices_for_tile (rendering.py:252-289) for one tile at any origin: d_indices receives
   min(cap, n) entries (-1 past the count), h_count (host) the count: one wait. */
int32_t gc_splat_indices_for_tile(gc_ctx* ctx, int64_t n, const double* d_means, const double* d_Sigmas_inv,
                                  int32_t origin_y, int32_t origin_x, int32_t tile_size, int32_t cap, double eps,
                                  int32_t* d_indices, int32_t* h_count);

/* render_tile_ewa (rendering.py:297-355) for one tile at any origin over the n_idx splats d_indices
   (int32, each clamped into [0, n)) in that order; n_idx = -1: every splat in index order. d_image
   (tile_size, tile_size, 3). n = 0 or n_idx = 0: a zero image (:324-327). No wait. */
int32_t gc_render_tile_ewa(gc_ctx* ctx, int64_t n, const double* d_means, const double* d_Sigmas_inv,
                           const double* d_alphas, const double* d_colors, int32_t origin_y, int32_t origin_x,
                           int32_t tile_size, const int32_t* d_indices, int64_t n_idx, double log_clip,
                           double* d_image);

/* fbm_at_splat_positions (rendering.py:212-228): d_out (n) from d_xy (n, 2). Domain of the integer
   hash as in gc_bev_splat_prep. No wait. */
int32_t gc_fbm_at_positions(gc_ctx* ctx, int64_t n, const double* d_xy, int32_t octaves, double gain, int64_t seed,
                            double* d_out);

/* ------------------------------------------------------------------------------------------
 * The camera view of the map: perspective splats, depth-ordered tile lists, front-to-back compositing
 * (tools/view_splat_jaxsplat.py around jaxsplat.render_v2; the raster itself is this build's).
 * ------------------------------------------------------------------------------------------ */
/* CameraViewConfig */
typedef struct {
  double near; /* near and far are macros of some toolchains' system headers (windows.h): #undef them there */
  double far;
  double lowpass_px2;
  double radius_sigma;
  double alpha_floor;
  double alpha_max;
  double alpha_skip;
  double t_stop;
  double bg_r; /* the background colour */
  double bg_g;
  double bg_b;
  double shade; /* 0 or 1 */
  double eps;
} gc_camview_cfg;
/* The 2D splats of n_views camera views of n primitives, view-major. The caller allocates every array. */
typedef struct gc_cam_splats {
  double* means_px;   /* (n_views, n, 2) column, row */
  double* Sigmas_inv; /* (n_views, n, 2, 2) */
  double* depths;     /* (n_views, n) camera z; +inf where not valid */
  double* radii;      /* (n_views, n) pixels */
  double* alphas;     /* (n) the same for every view */
  double* colors;     /* (n_views, n, 3) */
  uint8_t* valid;     /* (n_views, n) */
} gc_cam_splats;

/* Rows [0, n) of a batch as the 2D splats of n_views pinhole views, view v with h_T_cw[v] (4, 4, row-major,
   camera from world: p = R mu + t) and h_intrinsics[v] = (fx, fy, cx, cy) (host), for H x W images:
   valid where p and Sigma_world are finite and near < p.z < far (strict); means_px =
   (fx x / z + cx, fy y / z + cy); Sigma_px = sym(M Sigma M^T) + lowpass_px2 I with M = J R and
   J = [[fx/z, 0, -fx tx/z^2], [0, fy/z, -fy ty/z^2]] at the clamped tangents
   tx = clamp(x/z, +-1.3 max(cx, W - cx)/fx) z, ty likewise with cy, H, fy; Sigmas_inv = its closed-form
   inverse (det = ad - b^2 of the symmetrised matrix); radii = radius_sigma sqrt(lambda_max(Sigma_px));
   depths = p.z; colors = color * vmf_shading_multi_lobe(eta) for the unit direction from the primitive
   to the camera centre -R^T t (shade = 0: color itself); an invalid row has depth +inf and zeros
   elsewhere. alphas = clip(mass / m_max, alpha_floor, 1), m_max the largest positive mass of the n rows
   (1 if none), reduced on the device (view_splat_jaxsplat.py:108-111). No wait; uses the context's
   scratch. GC_ERR_ARG before any launch for n outside [0, 2^24], n_views outside [1, 32], n_lobes
   outside [1, 8], H or W outside [1, 16384], fx or fy <= 0, a non-finite host value, a bottom row of
   T_cw other than (0, 0, 0, 1), max |R^T R - I| > 1e-9, near <= 0, far <= near, alpha_max outside
   (0, 1] or NULL pointers. n = 0 launches nothing. */
int32_t gc_camera_splat_prep(gc_ctx* ctx, const gc_render_batch* batch, int64_t n, int32_t n_views, const double* h_T_cw,
                             const double* h_intrinsics, int32_t H, int32_t W, const gc_camview_cfg* cfg,
                             const gc_cam_splats* out);

/* The tile lists and the composited images of camera splats. Tiles as in gc_render_ewa_tiles: tile
   (ty, tx) covers the pixels [tx ts, (tx + 1) ts) x [ty ts, (ty + 1) ts). A valid splat survives where
   mx + r > x0, mx - r < x0 + ts, my + r > y0 and my - r < y0 + ts (all strict); a tile's list is the
   first cap of its survivors in the order (depth ascending, index ascending): d_tile_survivors
   (n_views, T) the number before the cut, d_tile_counts = min(survivors, cap), d_tile_indices
   (n_views, T, cap), -1 past the count. Per pixel centre (column + 0.5, row + 0.5), from T = 1,
   C = D = 0, n = 0, for each list entry in order: q = d^T Sigma_inv d, a = min(alpha_max,
   alpha exp(-max(q, 0) / 2)); a < alpha_skip is skipped; else C += T a color, D += T a depth, n += 1,
   T *= 1 - a, and the pixel stops once T < t_stop (the entry that crossed is composited). d_images
   (n_views, H, W, 3) = C + T background, d_alpha (n_views, H, W) = 1 - T, d_depth = D / (1 - T) where
   1 - T > eps, else 0, d_n_contrib (int32) = n. Bitwise reproducible. No wait. n = 0: empty lists from
   memsets and the background image. GC_ERR_ARG before any launch for tile_size outside [1, 32], H or W
   not a multiple of tile_size in [1, 16384], cap outside [1, 256], n < 0, n_views outside [1, 32], a
   non-finite configuration value, near <= 0, far <= near, alpha_max outside (0, 1],
   n_views * T * n >= 2^32 or NULL pointers. */
int32_t gc_render_depth_tiles(gc_ctx* ctx, int32_t n_views, int64_t n, const gc_cam_splats* splats, int32_t H, int32_t W,
                              int32_t tile_size, int32_t cap, const gc_camview_cfg* cfg, double* d_images,
                              double* d_alpha, double* d_depth, int32_t* d_n_contrib, int32_t* d_tile_counts,
                              int32_t* d_tile_survivors, int32_t* d_tile_indices);

/* ------------------------------------------------------------------------------------------
 * Depth pose evidence from the camera view: the rendered depth against an observed depth image,
 * linearised in the pose by forward-mode tangents carried through the compositing (this build's,
 * DESIGN.md §4, "Depth pose evidence").
 *
 * The tangent convention is visual_pose_evidence.py's (r = map - (R m + t) with d/dt = -I, :89-99;
 * R_delta = R_scatter R_pred^T, :234-238): a world-frame decoupled perturbation delta = [dt, dtheta] of
 * the body pose, t_wb' = t_wb + dt, R_wb' = Exp(dtheta) R_wb, so that L and h add to
 * gc_visual_pose_evidence's in the same coordinates. With T_cw = inv(T_wb T_bc), R = R_cw,
 * p = R mu + t_cw and e_k the k-th unit vector: dp/ddt_k = -R e_k, dp/ddtheta_k = R [mu - t_wb]x e_k,
 * dR_cw/ddtheta_k = -R [e_k]x, dR_cw/ddt = 0.
 * ------------------------------------------------------------------------------------------ */
#define GC_DEPTHEV_PARTS 46   /* per pose: L6 (36, row-major) | h6 (6) | cost | n_used | sum_cov | sum_w */
#define GC_DEPTHEV_PARTIAL 31 /* per (pose, tile): the 21 upper entries of w J J^T by rows | w J r (6) | cost |
                                 n_used | sum_cov | sum_w */

/* The six pose tangents of gc_camera_splat_prep's outputs, per (pose, primitive): h_T_cw and
   h_intrinsics as that entry takes them (the same arrays), h_t_wb (n_poses, 3) the body positions the
   rotations turn about (host); splats the prep's outputs for these views. With dp = (dx, dy, dz):
   d_dmeans_px (n_poses, n, 6, 2) = (fx (dx/z - x dz/z^2), fy (dy/z - y dz/z^2)); d_ddepths
   (n_poses, n, 6) = dz; d_dSigmas_inv (n_poses, n, 6, 3), the entries 00, 01, 11 of
   -Sigma_inv dSigma_px Sigma_inv with dSigma_px = sym(dM Sigma M^T + M Sigma dM^T), dM = dJ R + J dR,
   dJ00 = -fx dz/z^2, dJ02 = -fx (dtx/z^2 - 2 tx dz/z^3), dtx = dx where the tangent is not clamped and
   +-lim dz where it is (the y row likewise); the low-pass term has no derivative. Rows that are not
   valid are zero. No wait. GC_ERR_ARG before any launch for n outside [0, 2^24], n_poses outside
   [1, 32], H or W outside [1, 16384], fx or fy <= 0, a non-finite host value, a bottom row of T_cw
   other than (0, 0, 0, 1), max |R^T R - I| > 1e-9 (extrinsics that are no rotation show here), an
   invalid configuration or NULL pointers. n = 0 launches nothing. */
int32_t gc_camera_splat_jvp(gc_ctx* ctx, const gc_render_batch* batch, int64_t n, int32_t n_poses, const double* h_T_cw,
                            const double* h_t_wb, const double* h_intrinsics, int32_t H, int32_t W,
                            const gc_camview_cfg* cfg, const gc_cam_splats* splats, double* d_dmeans_px,
                            double* d_ddepths, double* d_dSigmas_inv);

/* Gaussian pose evidence of an observed depth image d_depth_obs (H, W; float32, metres, device; shared
   by the poses) against the rendered depth, per pose, over the lists d_tile_counts / d_tile_indices and
   beside the images d_alpha / d_depth that gc_render_depth_tiles made for the same arguments. One
   workgroup per (pose, tile), one thread per pixel (tile_size <= 16); compositing in list order with
   that entry's branches (raw = alpha exp(-max(q, 0) / 2), a = min(alpha_max, raw), skipped below
   alpha_skip, stop once T < t_stop), the state (T, D, dT[6], dD[6]) in registers:
   dq = -2 d^T Sigma_inv dmean + d^T dSigma_inv d; da = -a dq / 2, or 0 where raw > alpha_max or q < 0;
   dD += dT a z + T da z + T a dz; dT <- dT (1 - a) - T da. Branches, lists and their order are constants
   of the linearisation. With A = d_alpha and the rendered depth d_depth, a pixel is used where
   depth_obs is finite, min_depth < depth_obs < max_depth (strict) and A > eps; there
   J = (dD A + D dT) / A^2, r = depth - depth_obs, sigma = sigma0 + slope depth_obs (depth_model 0) or
   sigma0 + slope depth_obs^2 (1), u = (nu + 1) / (nu + (r / sigma)^2) (use_robust 0: u = 1),
   w = A u / sigma^2 (a constant of the linearisation). L6 = sum w J J^T, h6 = -sum w J r,
   cost = sum w r^2, n_used, sum_cov = sum A, sum_w = sum w over the used pixels: per tile by a
   fixed-order workgroup sum, over the tiles in tile order; no atomics, bitwise reproducible.
   d_parts (n_poses, GC_DEPTHEV_PARTS). accumulate 0: d_L_pose (n_poses, 22, 22) = L6 + eps_lift I in
   [0:6, 0:6] and zeros elsewhere, d_h_pose (n_poses, 22) = h6 in [0:6] and zeros; accumulate 1: L6 and h6
   are added into the caller's d_L_pose and d_h_pose, no lift, nothing else touched. d_residual and
   d_weight (n_poses, H, W; either may be NULL) receive r and w, zero where the pixel is not used.
   No wait; uses the context's scratch. n = 0: no raster; the no-pixel outputs (L6 = 0, h6 = 0).
   GC_ERR_ARG before any launch for n_poses outside [1, 32], tile_size outside [1, 16], H or W not a
   multiple of tile_size in [1, 16384], cap outside [1, 256], n < 0, an invalid configuration,
   depth_model not 0 or 1, sigma0 <= 0, slope < 0, min_depth >= max_depth or min_depth < 0, use_robust
   with nu <= 0, a non-finite parameter, eps_lift < 0, n_poses * T * n >= 2^32 or NULL pointers. */
int32_t gc_depth_pose_evidence(gc_ctx* ctx, int32_t n_poses, int64_t n, const gc_cam_splats* splats,
                               const double* d_dmeans_px, const double* d_ddepths, const double* d_dSigmas_inv,
                               int32_t H, int32_t W, int32_t tile_size, int32_t cap, const gc_camview_cfg* cfg,
                               const int32_t* d_tile_counts, const int32_t* d_tile_indices, const double* d_alpha,
                               const double* d_depth, const float* d_depth_obs, int32_t depth_model, double sigma0,
                               double slope, double min_depth, double max_depth, int32_t use_robust, double robust_nu,
                               double eps_lift, int32_t accumulate, double* d_L_pose, double* d_h_pose,
                               double* d_parts, double* d_residual, double* d_weight);

/* ------------------------------------------------------------------------------------------
 * Photometric pose evidence from the camera view: one luminance channel of the rendered colour against
 * an observed image, in the depth evidence's tangent convention, coordinates and output layout (this
 * build's, DESIGN.md §4, "Photometric pose evidence"). The luminance of a colour (r, g, b) is
 * y = (w_r r + w_g g) + w_b b for a weight triple w (host, 3 doubles; any finite values; the keypoint
 * detector's grey is (4899, 9617, 1868) / 16384). The residual is against Y / A, the rendered luminance
 * over the coverage, as the rendered depth is D / A: it does not read the background colour.
 * ------------------------------------------------------------------------------------------ */

/* d_rgb8 (H, W, 3) uint8 as d_lum (H, W) float32 = ((w_r R + w_g G) + w_b B) / 255, the sum in f64. No
   wait. GC_ERR_ARG before the launch for H or W outside [1, 16384], a non-finite weight or NULL pointers. */
int32_t gc_image_luminance(gc_ctx* ctx, const uint8_t* d_rgb8, int32_t H, int32_t W, const double* h_weights,
                           float* d_lum);

/* The luminance of gc_camera_splat_prep's colour rows and its six pose tangents, per (pose, primitive);
   the arguments as gc_camera_splat_jvp takes them. d_lum (n_poses, n) = y of splats->colors (the forward's
   bits, shading included). d_dlum (n_poses, n, 6) = (w . batch->color) ds_k with ds the tangent of the vMF
   shading at vd = c - mu, c the camera centre: dc = e_k for dt_k and e_k x (c - t_wb) for dtheta_k;
   n = |vd|, nv = n + 1e-12, v = vd / nv, dv = dc / nv - vd (vd . dc) / (n nv^2);
   ds = (1 / (1 + mean kappa)) (1 / L) sum_l exp(kappa_l (m_l . v - 1)) kappa_l (m_l . dv) with
   m_l = eta_l / (kappa_l + 1e-12), kappa_l = |eta_l| (a lobe with eta = 0 contributes 0). Rows that are not
   valid have lum = 0 and dlum = 0; shade = 0 gives dlum = 0. No wait. GC_ERR_ARG before any launch for what
   gc_camera_splat_jvp refuses, n_lobes outside [1, 8], a non-finite weight or NULL pointers. n = 0
   launches nothing. */
int32_t gc_camera_shade_jvp(gc_ctx* ctx, const gc_render_batch* batch, int64_t n, int32_t n_poses, const double* h_T_cw,
                            const double* h_t_wb, const double* h_intrinsics, int32_t H, int32_t W,
                            const gc_camview_cfg* cfg, const gc_cam_splats* splats, const double* h_weights, double* d_lum,
                            double* d_dlum);

/* Gaussian pose evidence of an observed luminance image d_lum_obs (H, W; float32, NaN or an infinity
   marks a hole; device; shared by the poses), per pose, over the lists and beside the coverage d_alpha of
   gc_render_depth_tiles, with gc_depth_pose_evidence's raster, branches and order and the state
   (T, Y, dT[6], dY[6]): Y += T a y; dY += dT a y + T da y + T a dy (y, dy: gc_camera_shade_jvp's). A pixel
   is used where lum_obs is finite and A > eps; there r = Y / A - lum_obs, J = (dY A + Y dT) / A^2,
   u = (nu + 1) / (nu + (r / sigma)^2) (use_robust 0: u = 1), w = A u / sigma^2. L6, h6, cost, n_used,
   sum_cov, sum_w, d_parts (n_poses, GC_DEPTHEV_PARTS), d_L_pose, d_h_pose, accumulate, d_residual and
   d_weight as in gc_depth_pose_evidence; d_lum_render (n_poses, H, W; may be NULL) receives Y / A, 0 where
   A <= eps. No wait; uses the context's scratch; bitwise reproducible. n = 0: no raster. GC_ERR_ARG
   before any launch for that entry's frame bounds, an invalid configuration, sigma <= 0, use_robust with
   nu <= 0, a non-finite parameter, eps_lift < 0 or NULL pointers. */
int32_t gc_photo_pose_evidence(gc_ctx* ctx, int32_t n_poses, int64_t n, const gc_cam_splats* splats,
                               const double* d_dmeans_px, const double* d_dSigmas_inv, const double* d_lum,
                               const double* d_dlum, int32_t H, int32_t W, int32_t tile_size, int32_t cap,
                               const gc_camview_cfg* cfg, const int32_t* d_tile_counts, const int32_t* d_tile_indices,
                               const double* d_alpha, const float* d_lum_obs, double sigma, int32_t use_robust,
                               double robust_nu, double eps_lift, int32_t accumulate, double* d_L_pose, double* d_h_pose,
                               double* d_parts, double* d_lum_render, double* d_residual, double* d_weight);

/* Both evidences in one pass over the lists (q, the exponential, dq and da are shared): the arguments of
   gc_depth_pose_evidence and of gc_photo_pose_evidence. d_parts (n_poses, 2, GC_DEPTHEV_PARTS): the depth
   row, then the luminance row, each the bytes of its own entry. The depth's L6 and h6 and then the
   luminance's are added into d_L_pose / d_h_pose, two successive additions in that order; accumulate 0:
   one eps_lift I is added, with the depth's. The same bytes as gc_depth_pose_evidence followed by
   gc_photo_pose_evidence with accumulate 1. GC_ERR_ARG as either entry. */
int32_t gc_rgbd_pose_evidence(gc_ctx* ctx, int32_t n_poses, int64_t n, const gc_cam_splats* splats,
                              const double* d_dmeans_px, const double* d_ddepths, const double* d_dSigmas_inv,
                              const double* d_lum, const double* d_dlum, int32_t H, int32_t W, int32_t tile_size,
                              int32_t cap, const gc_camview_cfg* cfg, const int32_t* d_tile_counts,
                              const int32_t* d_tile_indices, const double* d_alpha, const double* d_depth,
                              const float* d_depth_obs, int32_t depth_model, double sigma0, double slope, double min_depth,
                              double max_depth, int32_t depth_use_robust, double depth_robust_nu, const float* d_lum_obs,
                              double lum_sigma, int32_t lum_use_robust, double lum_robust_nu, double eps_lift,
                              int32_t accumulate, double* d_L_pose, double* d_h_pose, double* d_parts, double* d_residual,
                              double* d_weight, double* d_lum_render, double* d_lum_residual, double* d_lum_weight);

#ifdef __cplusplus
}
#endif
#endif /* GCSLAM_H_ */
