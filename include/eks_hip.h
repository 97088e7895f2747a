/*
 * eks_hip.h -- C ABI of libeks_hip.so, the MI355X (gfx950) ensemble Kalman
 * smoother.  Plain pointers and sizes only: no torch or numpy types.
 *
 * The reference (erialc-cal/eks, Python) has no FFI; its boundary is the four
 * Python functions of eks/ensemble_kalman.py.  Each entry point below states
 * which of them it replaces.  The Python package eks_amd binds these symbols
 * with ctypes (see INTEGRATION.md for the binding a maintainer of the
 * reference would add).
 *
 * Conventions
 *   - Every array argument is a DEVICE pointer (hipMalloc'd / torch cuda
 *     memory) unless the comment says otherwise.  Calls are stream-ordered on
 *     `stream` (a hipStream_t passed as void*; NULL = the null stream) and do
 *     not synchronise; they never allocate, so they can be captured in a
 *     hipGraph.
 *   - Floating point is float64 ("f64") throughout the recursions; member
 *     observations may be f32 or f64 (EKS_F32 / EKS_F64).
 *   - Matrices are row-major.  Batched arrays carry a leading trajectory
 *     index b in [0, B); a "trajectory" is one (video, keypoint) series.
 *   - Return value: EKS_OK or an error code; eks_last_error() gives the text
 *     (thread-local).  Numerical failures are reported per trajectory in the
 *     optional int32 `status` array (device, length B), a bit mask:
 *       0 = ok
 *       EKS_STATUS_SINGULAR   a matrix the reference would hand to
 *                             np.linalg.solve was singular (the reference
 *                             raises LinAlgError there)
 *       EKS_STATUS_BAD_MODEL  a model_flags promise (A or C = identity, the
 *                             pupil structure) does not hold for this
 *                             trajectory's parameters
 *       EKS_STATUS_SCAN       the time-parallel scan could not form a chunk
 *                             summary (singular Q with exact observations);
 *                             rerun that batch with algo = 1
 *     More than r exact columns in one frame is the reference's singular S.
 *     It is flagged only when a pivot rounds to <= 0.
 *     NaNs propagate exactly as in numpy and are not an error.
 */
#ifndef EKS_HIP_H
#define EKS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  EKS_OK = 0,
  EKS_ERR_ARG = 1,         /* bad size / NULL pointer / bad mode */
  EKS_ERR_UNSUPPORTED = 2, /* (r, n, E) combination not compiled in */
  EKS_ERR_HIP = 4          /* a HIP runtime call failed */
};

/* per-trajectory status bits */
enum { EKS_STATUS_SINGULAR = 1, EKS_STATUS_BAD_MODEL = 2, EKS_STATUS_SCAN = 4 };

/* model structure promises for eks_smooth (verified per trajectory) */
enum { EKS_MODEL_A_IDENTITY = 1, EKS_MODEL_C_IDENTITY = 2, EKS_MODEL_PUPIL = 4 };

enum { EKS_F32 = 0, EKS_F64 = 1 };
/* eks_smooth input that is not member predictions but the ensemble output
 * itself, as written by eks_fit (yev != NULL): y / ev planes, y float32
 * (EKS_YEV32) or float64 (EKS_YEV64); see eks_yev_bytes. */
enum { EKS_YEV32 = 2, EKS_YEV64 = 3 };
enum { EKS_MEDIAN = 0, EKS_MEAN = 1 };

/* Last error message of the calling thread ("" if none). */
const char *eks_last_error(void);

/* Library ABI version (major*100 + minor). */
int eks_version(void);

/* Largest state / observation / ensemble sizes the kernels accept. */
int eks_max_latent(void);
int eks_max_obs(void);
int eks_max_members(void);

/*
 * eks_ensemble -- replaces eks/ensemble_kalman.py:4-57 `ensemble()`.
 *
 * Member observation x(b, t, e, j) is read from
 *     obs[b*sb + t*st + e*se + j*sj]      (strides in ELEMENTS, any layout)
 * for b < B, t < T, e < E, j < n.  For every (b, t, j):
 *     preds = median_e x   (mode EKS_MEDIAN; mean of the two middle values
 *                            for even E, as np.median)  or  mean_e x
 *     vars  = var_e(x, ddof=0) / E     (in both modes, quirk of :46)
 * A NaN among the members makes both outputs NaN (np.median / np.var).
 * preds / vars: (B, T, n) contiguous f64.
 */
int eks_ensemble(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n,
                 int64_t sb, int64_t st, int64_t se, int64_t sj, int mode,
                 double *preds, double *vars, void *stream);

/*
 * eks_forward -- replaces eks/ensemble_kalman.py:59-107 `filtering_pass()`
 * (and the kalman_dot calls it makes, :110-117), batched over B trajectories.
 *
 * Inputs (all f64, contiguous):
 *   y  (B, T, n)   observations        ev (B, T, n)  ensemble variances
 *   m0 (B, r)      S0 (B, r, r)        A (B, r, r)   Q (B, r, r)   C (B, n, r)
 *   R  (B, n, n) or NULL: the caller's R matrix.  As in the reference its
 *      diagonal is replaced by ev[t] at every step; NULL means R is diagonal.
 *      This function does not write R (the Python shim reproduces the
 *      in-place mutation on the host).
 *   params_shared: if nonzero, m0/S0/A/Q/C/R hold ONE trajectory's values
 *      used for all b (batch stride 0).
 * Outputs (any may be NULL):
 *   mf (B, T, r)   Vf (B, T, r, r)   S (B, T, r, r) -- S[t] = A Vf[t] A^T + Q,
 *      the covariance predicted for step t+1; S[T-1] = 0 as in the reference.
 *   nll (B) -- the Gaussian innovation negative log-likelihood
 *      (the reference has no counterpart).
 *   status (B) int32 -- see above.
 */
int eks_forward(int64_t B, int64_t T, int n, int r, const double *y, const double *ev,
                const double *m0, const double *S0, const double *A, const double *Q,
                const double *C, const double *R, int params_shared, double *mf, double *Vf,
                double *S, double *nll, int32_t *status, void *stream);

/*
 * eks_backward -- replaces eks/ensemble_kalman.py:120-164 `smooth_backward()`.
 *   mf (B,T,r), Vf (B,T,r,r), S (B,T,r,r), A (B,r,r) (shared if params_shared)
 *   -> ms (B,T,r), Vs (B,T,r,r), CV (B,T-1,r,r); any output may be NULL.
 * J_t = solve(S[t], A Vf[t])^T, exactly as :158 (Q, C and y are unused by
 * the reference and are not arguments here).
 */
int eks_backward(int64_t B, int64_t T, int r, const double *mf, const double *Vf,
                 const double *S, const double *A, int params_shared, double *ms, double *Vs,
                 double *CV, int32_t *status, void *stream);

/*
 * eks_kalman_dot -- replaces eks/ensemble_kalman.py:110-117 `kalman_dot()`:
 *   out (r, k) = V C^T (R + C V C^T)^{-1} x,  x (n, k), V (r, r), C (n, r), R (n, n).
 * k = 1 for the vector form.  Single problem, f64.
 */
int eks_kalman_dot(int n, int r, int k, const double *x, const double *V, const double *C,
                   const double *R, double *out, int32_t *status, void *stream);

/*
 * Packed per-trajectory model for the fused smoother: for each b, P doubles
 *   [ m0 (r) | S0 (r*r) | A (r*r) | Q (r*r) | C (n*r) | offset (n) ]
 * with P = eks_param_len(n, r).  `offset` is added to C ms[t] on output (the
 * camera / keypoint means the wrappers subtract before filtering and add back
 * after: eks/multiview_pca_smoother.py:698-700, :756-765;
 * eks/pupil_smoother.py:158-172, :197).
 */
int64_t eks_param_len(int n, int r);

/*
 * eks_smooth -- the fused hot path: ensemble (eks_ensemble) -> centre
 * (y = preds - offset) -> forward filter -> RTS backward -> projection
 * out = C ms + offset, i.e. eks/ensemble_kalman.py:4-164 plus
 * eks/multiview_pca_smoother.py:745 / eks/pupil_smoother.py:190, in one call
 * for B trajectories with R diagonal (R_t = diag(ev[t])).
 *
 *   obs      member observations, strides as eks_ensemble
 *   params   (B, P) f64 packed models (see eks_param_len)
 *   out      smoothed observations out(b,t,j) = out[b*ob + t*ot + j*oj] (f64);
 *            NULL = filter only: just the NLL (requires nll, ms must be NULL),
 *            e.g. to score candidate models in a parameter sweep
 *   ms       (B, T, r) contiguous smoothed latents, or NULL
 *   nll      (B) or NULL
 *   model_flags  EKS_MODEL_A_IDENTITY / EKS_MODEL_C_IDENTITY: the caller
 *            promises A = I (and C = I, r = n) for every trajectory, which
 *            selects kernels that skip those products (single-view: both;
 *            multi-camera: A).  EKS_MODEL_PUPIL (r = 3, n = 8): C is the
 *            pupil measurement matrix of eks/pupil_smoother.py:150-153 (rows
 *            in the order top x, y, bottom x, y, right x, y, left x, y) and A,
 *            Q are diagonal (:140-147): sparse updates, the two pairs of
 *            equal rows folded into one observation each.  Violations are
 *            flagged in `status` by the compiled kernels (algos 1-3).  The
 *            runtime-n kernel (algo 4) runs the general model whatever the
 *            flags say: it neither uses nor checks them, so it never sets
 *            EKS_STATUS_BAD_MODEL (its results are those of the general
 *            model, i.e. correct for any A, C).
 *   workspace / workspace_bytes: device scratch of at least
 *            eks_smooth_workspace_bytes(...) bytes (not zeroed by caller).
 *   algo     0 = automatic, 1 = sequential (one lane per trajectory),
 *            2 = time-parallel chunked scan, three passes,
 *            3 = time-parallel, two passes over the members (chunk-level RTS
 *            maps; smoothing only: a filter-only call runs algo 2; needs
 *            E in 3..5 or y / ev planes, else algo 2),
 *            4 = the runtime-n kernels (any n <= 64, r = 2 or 3, members or
 *            y / ev planes): what every (r, n) without compiled kernels runs --
 *            (2, 2) and (3, 4|6|8|12|16) are compiled; e.g. the multi-camera model
 *            with V = 5, 7 or V > 8 cameras, n = 2V (the reference accepts any V:
 *            eks/multiview_pca_smoother.py:641-666).  eks_smooth_algo
 *            reports 4 for those shapes.  Many trajectories: one GPU lane
 *            per trajectory, sequential in time; few long ones: algo 2's
 *            time-parallel chunk scan with the n observation rows streamed
 *            one at a time (EKS_DBG_RT_FORM below).
 *   status   (B) int32, REQUIRED; zeroed by the call, then bit flags as above.
 */
size_t eks_smooth_workspace_bytes(int64_t B, int64_t T, int n, int r, int E, int algo);
int eks_smooth(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n, int r,
               int64_t sb, int64_t st, int64_t se, int64_t sj, int mode, const double *params,
               double *out, int64_t ob, int64_t ot, int64_t oj, double *ms, double *nll,
               void *workspace, size_t workspace_bytes, int model_flags, int algo,
               int32_t *status, void *stream);

/* Chunk length the time-parallel algorithm uses for (B, T, r) (0 if algo 1
 * would be chosen automatically).  Exposed for tests and DESIGN.md. */
int64_t eks_smooth_chunk_len(int64_t B, int64_t T, int r);

/* The algorithm (1, 2 or 3) an eks_smooth call with these arguments runs
 * (smoothing calls; a filter-only call that resolves to 3 runs 2).  Exposed
 * for the bench line and tests. */
int eks_smooth_algo(int64_t B, int64_t T, int n, int r, int E, int algo);

/* Tests and DESIGN.md: the kernel forms an eks_smooth call of this size takes.
 * Host only, launches nothing.  Fills up to n_info int64 values, returns how many it defines.
 * The values come from the launcher's own plan functions, in this order:
 *   EKS_PLAN_ALGO       the algorithm the call runs (as eks_smooth_algo; a filter-only
 *                       call that resolves to 3 runs 2).  Algos 1 and 4 define only this.
 *   algo 2 (the three-pass chunked scan) defines the next nine:
 *   EKS_PLAN_L          chunk length in steps (a smoothing call of few trajectories
 *                       uses shorter chunks than a filter-only one)
 *   EKS_PLAN_NC         chunks per trajectory, ceil(T / L)
 *   EKS_PLAN_LS         checkpoint interval of K3 / K5 within a chunk
 *   EKS_PLAN_UNIFORM    1: whole 256-lane blocks per chunk (the uniform-lane kernels)
 *   EKS_PLAN_WAVE_SCAN  1: the wave-parallel chunk scans, 0: the serial ones
 *   EKS_PLAN_GRP        1: group mode (in-block scans in K1 / K3, K2 / K4 over groups)
 *   EKS_PLAN_JD         1: K3 stores the (J, d) planes and k_c5_jd reads them
 *   EKS_PLAN_G          blocks per trajectory of the chunk scans as launched
 *                       (over the groups in group mode; 1 for the serial scans)
 *   EKS_PLAN_NG         groups per trajectory in group mode, else 0
 *   algo 3 (two passes) leaves those nine 0 and defines:
 *   EKS_PLAN_FINE_LEN   fine chunk length in steps
 *   EKS_PLAN_NCF        fine chunks per trajectory
 *   EKS_PLAN_NCC        units of the backward pass (4 fine chunks each)
 *   EKS_PLAN_NCU        units of the forward pass (4 fine chunks; 8 at r = 2)
 *   EKS_PLAN_NGRP3      64-trajectory groups
 * `smoothing` is nonzero for a call with out != NULL.  Returns 0 for
 * non-positive sizes, an unknown algo or a shape without kernels.  (eks_smooth
 * runs algo 2 in place of 3 when the member strides do not fit algo 3's
 * 32-bit offsets; the query does not see strides.) */
enum {
  EKS_PLAN_ALGO = 0, EKS_PLAN_L = 1, EKS_PLAN_NC = 2, EKS_PLAN_LS = 3, EKS_PLAN_UNIFORM = 4,
  EKS_PLAN_WAVE_SCAN = 5, EKS_PLAN_GRP = 6, EKS_PLAN_JD = 7, EKS_PLAN_G = 8, EKS_PLAN_NG = 9,
  EKS_PLAN_FINE_LEN = 10, EKS_PLAN_NCF = 11, EKS_PLAN_NCC = 12, EKS_PLAN_NCU = 13,
  EKS_PLAN_NGRP3 = 14, EKS_PLAN_INFO_LEN = 15
};
int eks_smooth_plan_info(int64_t B, int64_t T, int n, int r, int E, int algo,
                         int smoothing /* out != NULL */, int64_t *info, int n_info);

/*
 * eks_smooth_var -- the posterior variances of eks_smooth's output: the
 * covariance recursions of eks/ensemble_kalman.py:59-164 alone (Vf, S, the
 * RTS gain and Vs do not depend on the observations), time-parallel over
 * chunks, with R_t = diag(ev[t]), ev the ensemble variances eks_smooth uses.
 *
 *   obs      member observations, strides as eks_ensemble (EKS_F32 / EKS_F64),
 *            or the y / ev hand-off planes of eks_fit (EKS_YEV32 / EKS_YEV64;
 *            strides ignored, only the ev planes are read)
 *   params   (B, P) f64 packed models (see eks_param_len); m0 and offset unused
 *   pvar     pvar(b,t,j) = c_j Vs_t c_j^T = pvar[b*vb + t*vt + j*vj] (f64), the
 *            variance of out(b,t,j); REQUIRED
 *   Vs       (B, T, r, r) contiguous smoothed covariances, or NULL
 *   status   (B) int32, REQUIRED; zeroed by the call.  EKS_STATUS_SINGULAR
 *            where the smoother's S_t is singular; EKS_STATUS_SCAN for a
 *            trajectory with an exact observation (ev[t][j] == 0: a single
 *            member or identical members), whose pvar / Vs are NaN -- run
 *            those through eks_ensemble / eks_forward / eks_backward.
 *            Other trajectories are unaffected; a NaN ev makes the
 *            trajectory NaN and is not an error.
 * r = 2 or 3, n <= 64 (the runtime-n smoother's limit), E <= eks_max_members(),
 * else EKS_ERR_UNSUPPORTED.  There are no model_flags: the general model runs.
 * eks_smooth_var_chunk_len: the chunk length as launched (a single chunk
 * covering T is the sequential form); EKS_DBG_PVAR_CHUNK forces it.
 */
size_t eks_smooth_var_workspace_bytes(int64_t B, int64_t T, int n, int r);
int64_t eks_smooth_var_chunk_len(int64_t B, int64_t T, int r);
int eks_smooth_var(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n, int r,
                   int64_t sb, int64_t st, int64_t se, int64_t sj, const double *params,
                   double *pvar, int64_t vb, int64_t vt, int64_t vj, double *Vs, void *workspace,
                   size_t workspace_bytes, int32_t *status, void *stream);

/*
 * eks_nll_sweep -- the innovation NLL (compute_nll; eks_smooth with out = NULL)
 * of K candidate models for each of B trajectories, in one call: the members
 * are read and reduced once for all candidates, and a candidate costs r
 * scalar updates per step whatever n is (the n observations of a step are
 * reduced to r scalar observations and a model-free constant).
 *
 *   obs      member observations, strides as eks_ensemble (EKS_F32 / EKS_F64),
 *            or the y / ev hand-off planes of eks_fit (EKS_YEV32 / EKS_YEV64;
 *            strides ignored)
 *   params   (K * B, P) f64 packed models (see eks_param_len): row k * B + b
 *            is candidate k of trajectory b.  The candidates of a trajectory
 *            may differ in m0, S0, A and Q; C and offset must equal
 *            candidate 0's bit for bit.
 *   nll      (K, B) f64, REQUIRED
 *   status   (K, B) int32, REQUIRED; zeroed by the call.  EKS_STATUS_SCAN on
 *            every candidate of a trajectory this path does not serve -- an
 *            exact observation (ev[t][j] == 0: a single member or identical
 *            members) or a C without full column rank (n < r included) -- whose
 *            NLLs are NaN: run those through eks_smooth with out = NULL.
 *            EKS_STATUS_BAD_MODEL on a row whose C or offset differ from
 *            candidate 0's; EKS_STATUS_SINGULAR where the filter's innovation
 *            variance is not positive.  Other trajectories are unaffected; a
 *            NaN member makes the NLLs of its trajectory NaN and is not an error.
 * r = 2 or 3, n <= 64, E <= eks_max_members(), K * B <= 2^28, else
 * EKS_ERR_UNSUPPORTED (the size queries return 0).  B = 0 or K = 0: EKS_OK,
 * nothing launched.  Results are bit-reproducible.
 * eks_nll_sweep_chunk_len: the chunk length as launched (a single chunk
 * covering T is the sequential form); EKS_DBG_SWEEP_CHUNK forces it.
 */
size_t eks_nll_sweep_workspace_bytes(int64_t B, int64_t K, int64_t T, int n, int r);
int64_t eks_nll_sweep_chunk_len(int64_t B, int64_t K, int64_t T, int r);
int eks_nll_sweep(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n, int r,
                  int64_t sb, int64_t st, int64_t se, int64_t sj, int mode,
                  const double *params /* (K*B, P): row k*B+b = candidate k of trajectory b */,
                  int64_t K, double *nll /* (K, B) */, void *workspace, size_t workspace_bytes,
                  int32_t *status /* (K, B), required, zeroed by the call */, void *stream);

/*
 * eks_smooth_gaps -- the smoother through missing observations, time-parallel
 * over chunks in information form.  Column (t, j) of trajectory b is MISSING
 * iff its ensemble average or its ensemble variance is not finite (a NaN
 * member; a +-inf member; a non-finite y or ev of a hand-off); there is no
 * mask argument -- a caller who rejects a prediction writes NaN into it.  A
 * missing column is left out of the update (a frame with nothing observed is
 * a pure prediction), and out / pvar are written for EVERY (t, j), missing or
 * not: the interpolation and its variance.  With complete data the results
 * equal eks_smooth's / eks_smooth_var's to rounding.  Every other entry point
 * keeps its NaN propagation.
 *
 *   obs      member observations, strides as eks_ensemble (EKS_F32 / EKS_F64),
 *            or the y / ev hand-off planes of eks_fit (EKS_YEV32 / EKS_YEV64;
 *            strides ignored)
 *   mode     EKS_MEDIAN / EKS_MEAN (the ensemble average)
 *   params   (B, P) f64 packed models (see eks_param_len)
 *   out      out(b,t,j) = c_j ms_t + offset_j = out[b*ob + t*ot + j*oj] (f64); REQUIRED
 *   pvar     pvar(b,t,j) = c_j Vs_t c_j^T with out's strides, or NULL
 *   ms       (B, T, r) contiguous smoothed means, or NULL
 *   Vs       (B, T, r, r) contiguous smoothed covariances, or NULL
 *   nll      (B) the Gaussian innovation NLL over the observed entries (a frame
 *            with nothing observed adds 0), or NULL
 *   nobs     (B) int32 number of observed entries, or NULL
 *   status   (B) int32, REQUIRED; zeroed by the call.  EKS_STATUS_SCAN for a
 *            trajectory with an exact observation (an OBSERVED column with
 *            ev[t][j] == 0: a single member or identical members), whose
 *            outputs are NaN; EKS_STATUS_SINGULAR where S_t of the RTS gain or
 *            I + P J of a composition is singular (finite operands only).
 *            Other trajectories are unaffected.  A trajectory with nothing
 *            observed at all is not an error: its output is the prior carried
 *            forward, m_t = A^t m0.
 * r = 2 or 3, n <= 64, E <= eks_max_members(), else EKS_ERR_UNSUPPORTED (the
 * size queries return 0).  B = 0: EKS_OK, nothing launched.  There are no
 * model_flags: the general model runs.  Results are bit-reproducible.
 * eks_smooth_gaps_chunk_len: the chunk length as launched (a single chunk
 * covering T is the sequential form); EKS_DBG_GAPS_CHUNK forces it.
 */
size_t eks_smooth_gaps_workspace_bytes(int64_t B, int64_t T, int n, int r);
int64_t eks_smooth_gaps_chunk_len(int64_t B, int64_t T, int r);
int eks_smooth_gaps(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n, int r,
                    int64_t sb, int64_t st, int64_t se, int64_t sj, int mode, const double *params,
                    double *out, int64_t ob, int64_t ot, int64_t oj, /* REQUIRED */
                    double *pvar /* out's strides, or NULL */, double *ms /* (B,T,r) or NULL */,
                    double *Vs /* (B,T,r,r) or NULL */, double *nll /* (B) or NULL */,
                    int32_t *nobs /* (B) observed entries, or NULL */, void *workspace,
                    size_t workspace_bytes, int32_t *status, void *stream);

/*
 * eks_draws_gaps -- S joint draws per trajectory from the smoothing posterior
 * of eks_smooth_gaps (same inputs, missing rule, limits, error codes and
 * status bits), by backward sampling on the device.  With J_t, D_t of the RTS
 * pass (D_t = P_t - J_t S_t J_t^T), chol the lower Cholesky factor with
 * positive diagonal and z(b,s,t,.) ~ N(0, I_r):
 *     delta_{T-1} = chol(P_{T-1}) z_{T-1}
 *     delta_t     = J_t delta_{t+1} + chol(D_t) z_t,   t = T-2 .. 0
 *     x_t = ms_t + delta_t,   draws(b,s,t,j) = c_j x_t + offset_j
 * time-parallel over the chunks of eks_smooth_gaps (the same chunk length,
 * EKS_DBG_GAPS_CHUNK).  Consecutive frames of one draw are correlated as the
 * posterior is (Cov(x_t, x_{t+1} | Y) = J_t Vs_{t+1}), which pvar cannot give.
 *
 *   S        draws per trajectory.  B = 0 or S = 0: EKS_OK, nothing of the draw
 *            stage is launched and draws is untouched; S < 0: EKS_ERR_ARG.
 *   noise    z(b,s,t,i) = noise[b*zb + s*zs + t*zt + i] (f64, i contiguous), or
 *            NULL: the kernels generate z from `seed` (below) and no noise
 *            tensor is allocated or read
 *   draws    draws(b,s,t,j) = draws[b*db + s*ds + t*dt + j*dj] (f64); REQUIRED
 *   xdraws   (B, S, T, r) contiguous latent draws x_t, or NULL
 *   out, pvar  eks_smooth_gaps's, with the same values; both optional here
 *            (pvar has out's strides, so it needs out: else EKS_ERR_ARG)
 *   status   (B) int32, REQUIRED; zeroed by the call.  eks_smooth_gaps's bits,
 *            and EKS_STATUS_SINGULAR for a trajectory where a Cholesky pivot of
 *            D_t (or P_{T-1}) is not > 0 (a NaN pivot included): ALL draws of
 *            that trajectory are NaN, other trajectories are unaffected.
 * r = 2 or 3, n <= 64, E <= eks_max_members(), B * S <= 2^28, T <= 2^40, else
 * EKS_ERR_UNSUPPORTED (the size query returns 0).  Results are bit-reproducible
 * from call to call, and draw (b, s) has the same bits whatever S is and
 * whichever other draws are asked for; its noise z(b,s,.,.) does not depend on
 * B, S, the chunk length or the launch shape.
 *
 * Seeded noise (noise == NULL), also written out by eks_draws_noise: component
 * i of z(b,s,t,.) comes from block i / 2 of a counter-based generator,
 * Philox4x32-10 (Salmon et al., SC 2011; multipliers 0xD2511F53, 0xCD9E8D57,
 * key increments 0x9E3779B9, 0xBB67AE85):
 *     key     = (seed & 0xffffffff, seed >> 32)
 *     counter = (t & 0xffffffff, (t >> 32) | (block << 8), s, b)
 *     (x0, x1, x2, x3) = philox4x32_10(counter, key)
 *     k1 = (x0 << 21) | (x1 >> 11),  k2 = (x2 << 21) | (x3 >> 11)   (53 bits each)
 *     u1 = (k1 + 1) * 2^-53 in (0, 1],  u2 = k2 * 2^-53 in [0, 1)
 *     z[2 block]     = sqrt(-2 log u1) * cos(6.283185307179586 * u2)
 *     z[2 block + 1] = sqrt(-2 log u1) * sin(6.283185307179586 * u2)
 * (r = 3 drops the second value of block 1).  eks_draws_noise writes
 * z(b,s,t,i) to noise[b*zb + s*zs + t*zt + i] with the same device function,
 * so eks_draws_gaps(seed) and eks_draws_gaps(noise = eks_draws_noise(seed))
 * agree; under EKS_DBG_DRAWS_RAW it writes (double)k1, (double)k2 instead.
 */
size_t eks_draws_gaps_workspace_bytes(int64_t B, int64_t S, int64_t T, int n, int r);
int64_t eks_draws_gaps_chunk_len(int64_t B, int64_t T, int r);
int eks_draws_gaps(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n, int r,
                   int64_t sb, int64_t st, int64_t se, int64_t sj, int mode, const double *params,
                   int64_t S, const double *noise, int64_t zb, int64_t zs, int64_t zt,
                   uint64_t seed /* used iff noise == NULL */,
                   double *draws, int64_t db, int64_t ds, int64_t dt, int64_t dj, /* REQUIRED */
                   double *xdraws /* (B,S,T,r) or NULL */,
                   double *out, int64_t ob, int64_t ot, int64_t oj, double *pvar, /* or NULL */
                   void *workspace, size_t workspace_bytes, int32_t *status, void *stream);
int eks_draws_noise(int64_t B, int64_t S, int64_t T, int r, uint64_t seed, double *noise,
                    int64_t zb, int64_t zs, int64_t zt, void *stream);

/*
 * eks_nll_sweep_gaps -- eks_nll_sweep through missing observations: the
 * Gaussian innovation NLL over the OBSERVED entries (eks_smooth_gaps's nll and
 * its missing rule: column (t, j) is missing iff its ensemble average or
 * variance is not finite) of K candidate models for each of B trajectories in
 * one call.  The members are read and reduced once for all candidates, to the
 * information-form sums W_t, w_t, kappa_t (r (r + 1) / 2 + r + 1 doubles per
 * step), which may be rank-deficient (a camera out) or zero (a blink); a
 * candidate costs r x r work per step whatever n is.
 *
 *   obs      member observations, strides as eks_ensemble (EKS_F32 / EKS_F64),
 *            or the y / ev hand-off planes of eks_fit (EKS_YEV32 / EKS_YEV64;
 *            strides ignored)
 *   params   (K * B, P) f64 packed models (see eks_param_len): row k * B + b
 *            is candidate k of trajectory b.  The candidates of a trajectory
 *            may differ in m0, S0, A and Q; C and offset must equal
 *            candidate 0's bit for bit.
 *   nll      (K, B) f64, REQUIRED.  A trajectory with nothing observed has
 *            exactly 0.0 for every candidate.
 *   nobs     (B) int32 number of observed entries, or NULL
 *   status   (K, B) int32, REQUIRED; zeroed by the call.  EKS_STATUS_SCAN on
 *            every candidate of a trajectory with an exact observation (an
 *            OBSERVED column with ev[t][j] == 0), whose NLLs are NaN: there is
 *            no fallback, mark the column missing or widen its variance.
 *            EKS_STATUS_BAD_MODEL on a row whose C or offset differ from
 *            candidate 0's (that row only); EKS_STATUS_SINGULAR where I + P W
 *            of a step or I + P J of a composition is singular (finite
 *            operands only).  Other trajectories are unaffected.
 * r = 2 or 3, n <= 64, E <= eks_max_members(), K * B <= 2^28, else
 * EKS_ERR_UNSUPPORTED (the size queries return 0).  B = 0 or K = 0: EKS_OK,
 * nothing launched.  Results are bit-reproducible.
 * eks_nll_sweep_gaps_chunk_len: the chunk length as launched (a single chunk
 * covering T is the sequential form); EKS_DBG_GAPS_SWEEP_CHUNK forces it.
 */
size_t eks_nll_sweep_gaps_workspace_bytes(int64_t B, int64_t K, int64_t T, int n, int r);
int64_t eks_nll_sweep_gaps_chunk_len(int64_t B, int64_t K, int64_t T, int r);
int eks_nll_sweep_gaps(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n, int r,
                       int64_t sb, int64_t st, int64_t se, int64_t sj, int mode,
                       const double *params /* (K*B, P): row k*B+b = candidate k of trajectory b */,
                       int64_t K, double *nll /* (K, B) */, int32_t *nobs /* (B) or NULL */,
                       void *workspace, size_t workspace_bytes,
                       int32_t *status /* (K, B), required, zeroed by the call */, void *stream);

/*
 * Time-sharded smoothing (SURVEY.md §8(e) "shard the time axis"): the frames
 * of every trajectory are split into nseg contiguous segments, segment k on
 * rank k, and the chunked scan of eks_smooth runs per segment in three
 * phases with two exchanges of per-trajectory aggregates between them (the
 * reference has no equivalent: its smoother is one sequential loop,
 * eks/ensemble_kalman.py:59-164).  Per segment of T frames starting at t_base of
 * T_total, with the arguments of eks_smooth (obs/out point at the segment's
 * own frames):
 *   phase 1: seg_out (B, EL), EL = R*R + 2R + R(R+1) <- the segment's aggregate
 *            filtering element (A, b, C, eta, J; C and J packed) (zeroes status);
 *   -> all-gather the elements, eks_seg_combine(kind 0) -> state (B, R+R(R+1)/2)
 *   phase 2: seg_in = that state (NULL on segment 0); seg_out (B, R*R + R) <-
 *            the segment's aggregate smoothing map ms_in -> ms_first;
 *   -> all-gather the maps, eks_seg_combine(kind 1) -> mean (B, R)
 *            (filter only: out = NULL, nll != NULL -> nll = the segment's share,
 *            no map, no phase 3)
 *   phase 3: seg_in = the smoothed mean entering the next segment (NULL on
 *            the last); writes out, ms (B, T, r) if not NULL, and nll = the
 *            segment's share, whose sum over segments is eks_smooth's nll.
 * The workspace (eks_smooth_seg_workspace_bytes) must survive phases 1..3.
 * Results equal eks_smooth's to rounding (different association order).
 */
size_t eks_smooth_seg_workspace_bytes(int64_t B, int64_t T, int n, int r);
int eks_smooth_seg(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n, int r,
                   int64_t sb, int64_t st, int64_t se, int64_t sj, int mode,
                   const double *params, double *out, int64_t ob, int64_t ot, int64_t oj,
                   double *ms, double *nll, void *workspace, size_t workspace_bytes,
                   int model_flags, int32_t *status, int64_t t_base, int64_t T_total, int phase,
                   const double *seg_in, double *seg_out, void *stream);
/* kind 0: in = nseg gathered elements (nseg, B, EL) -> out = state entering
 * segment `self`; kind 1: in = gathered maps (nseg, B, R*R+R) -> out = mean
 * entering segment self+1 (zeros when self is last).  status may be NULL. */
int eks_seg_combine(int kind, int64_t B, int nseg, int self, int r, const double *in,
                    double *out, int32_t *status, void *stream);

/*
 * eks_newton_filter -- replaces eks/newton_eks.py:115-148
 * `kalman_newton_recursive(y, mu0, S0, A, B, ensemble_vars, E, max_iter)`
 * for B trajectories (one lane each): information-form filter with
 * q[0] = mu0, P0 = inv(S0), D_t = diag(ensemble_vars[t]), P carried over
 * between the max_iter iterations, q updated in place.
 *   y, ev   (B, T, n) f64 contiguous (centred observations, ensemble variances)
 *   mu0 (r), S0 (r, r), A (r, r), Bm (n, r), E (r, r): per trajectory
 *           (b-strided) or, with params_shared = 1, one model for all
 *   q       (B, T, r) f64 output
 *   status  (B) int32 or NULL: EKS_STATUS_SINGULAR where the reference's
 *           np.linalg.inv would raise (zero variance, singular S0 / info).
 * The reference's loss vector is identically 0 (q is updated in place), so
 * it is not produced here.
 */
int eks_newton_filter(int64_t B, int64_t T, int n, int r, const double *y, const double *ev,
                      const double *mu0, const double *S0, const double *A, const double *Bm,
                      const double *E, int params_shared, int max_iter, double *q,
                      int32_t *status, void *stream);

/*
 * eks_fit -- batched model fit (F2), replacing the per-keypoint host fit of
 * eks/multiview_pca_smoother.py:684-731 (kind EKS_FIT_MULTICAM: PCA with r
 * axes, r = 3 there) and the single-view model of SURVEY.md §8 A6 (kind
 * EKS_FIT_SINGLEVIEW, r == n): good frames = max_j ensemble variance <=
 * np.percentile(., quantile_keep); offset = mean of their ensemble
 * predictions; S0 = diag(var of the good latents); Q = smooth_param *
 * cov(diff(good latents)) (ddof 1); A = I; C = I or the principal axes.
 * Writes params (B, eks_param_len(n, r)) for eks_smooth.  obs and strides
 * as eks_smooth (T >= 2).  status (B) or NULL: EKS_STATUS_SINGULAR where no
 * frame was kept (NaN threshold).  workspace: eks_fit_workspace_bytes.
 * n even, 2 <= n <= 16 (coordinate pairs: single view, or 2V for V <= 8
 * cameras; n > 8 runs the wide kernels and needs EKS_FIT_MULTICAM with
 * r = 3; the per-keypoint multi-camera wrappers fit on the host for any V).
 */
enum { EKS_FIT_SINGLEVIEW = 1, EKS_FIT_MULTICAM = 2 };
size_t eks_fit_workspace_bytes(int64_t B, int64_t T, int n);
int eks_fit(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n, int r,
            int64_t sb, int64_t st, int64_t se, int64_t sj, int mode, int kind,
            double smooth_param, double quantile_keep, double *params, void *workspace,
            size_t workspace_bytes, int32_t *status, void *yev, void *stream);

/*
 * Ensemble hand-off from eks_fit to eks_smooth (fit + smooth reading the
 * member predictions once): with yev != NULL (eks_yev_bytes(B, T, n,
 * obs_dtype, E, mode) bytes of device memory) eks_fit also writes the
 * ensemble output -- y planes [t*n + j][b] (float32 when every y is a member
 * value: float32 members, median, E in {3, 5}; else float64), then ev planes
 * (float64) at a 256-byte aligned offset -- and eks_smooth called with
 * obs = yev and obs_dtype = eks_yev_dtype(obs_dtype, E, mode)
 * (EKS_YEV32 / EKS_YEV64; strides ignored) smooths from it.  Results are
 * bit-identical to eks_smooth on the members.
 */
int eks_yev_dtype(int obs_dtype, int E, int mode);
size_t eks_yev_bytes(int64_t B, int64_t T, int n, int obs_dtype, int E, int mode);

/*
 * eks_fit_gaps -- eks_fit through missing observations, with the missing
 * rule of eks_smooth_gaps taken per frame: frame t of a trajectory is
 * complete iff the ensemble average and the ensemble variance of all n
 * columns are finite (no NaN or +-inf member, no overflowing variance).
 * With M complete frames, the threshold is np.percentile(worst[complete],
 * quantile_keep) with worst_t = max_j ev[t, j] (numpy's linear rule on the M
 * values), a frame is kept iff it is complete and worst_t <= threshold, and
 * everything else is eks_fit's over the kept frames in frame order -- the
 * differences are those of consecutive KEPT frames whatever their distance
 * in time.  That is the host fit on preds[ok], ev[ok] with ok the complete
 * frames.  M = 0: status EKS_STATUS_SINGULAR, nkept 0; M = 1 or
 * quantile_keep = 0: one kept frame (offset its average, S0 = 0, Q NaN,
 * status 0).  On members without gaps params, status and the planes are
 * bit-identical to eks_fit's.
 * Arguments, limits and error codes as eks_fit, except that status (B) and
 * yev (eks_yev_bytes) are required: the hand-off planes are written for
 * every frame, non-finite where the frame is not complete, and are what
 * eks_smooth_gaps / eks_nll_sweep_gaps read (eks_yev_dtype).  ncomplete,
 * nkept (B) int32 or NULL: M and the number of kept frames.
 * workspace: eks_fit_gaps_workspace_bytes (0 for unsupported shapes).
 */
size_t eks_fit_gaps_workspace_bytes(int64_t B, int64_t T, int n);
int eks_fit_gaps(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n, int r,
                 int64_t sb, int64_t st, int64_t se, int64_t sj, int mode, int kind,
                 double smooth_param, double quantile_keep, double *params,
                 void *workspace, size_t workspace_bytes, int32_t *status, void *yev,
                 int32_t *ncomplete, int32_t *nkept, void *stream);
/*
 * The fit from planes: eks_fit_gaps also accepts obs_dtype = EKS_YEV32 /
 * EKS_YEV64.  obs is then a y / ev hand-off buffer for (B, T, n) -- written
 * by eks_fit, eks_fit_gaps or eks_ensemble_gaps -- and the strides, E and
 * mode are ignored.  yev must be NULL or equal to obs (anything else is
 * EKS_ERR_ARG); nothing is written to the planes.  A frame is complete iff
 * every y and ev of it is finite.  On planes that eks_fit_gaps wrote from
 * members, params, status, ncomplete and nkept are bit-identical to that call.
 */

/*
 * eks_ensemble_gaps -- the ensemble over the VALID members of each column.
 *
 * Members are read as in eks_ensemble (strides in elements).  Member e of
 * column (b, t, j) is valid iff it is finite: NaN, +inf and -inf are skipped.
 * With m valid members and m >= min_members:
 *     y  = nanmedian_e x  (EKS_MEDIAN: the middle valid value, or the mean of
 *                          the two middle ones for even m)  or  nanmean_e x
 *     ev = nanvar_e(x, ddof=0) / m        (eks_ensemble's "/ E" with the
 *                                          count that was actually used)
 * With m < min_members the column is missing: y = ev = NaN.  A column whose E
 * members are all valid has the bits of eks_ensemble and of the planes eks_fit
 * writes (E = 3, 4, 5, 8; another E agrees to an ulp of ev), so min_members =
 * E is the all-members rule of eks_fit_gaps / eks_smooth_gaps.  min_members = 1 is
 * allowed, but a single valid member gives ev = 0, which eks_smooth_gaps
 * reports as an exact observation (EKS_STATUS_SCAN): use min_members >= 2.
 *
 * yev (required): EKS_YEV64 hand-off planes, eks_yev_bytes(B, T, n, EKS_F64,
 * E, mode) bytes -- y float64 at [t*n + j][b], then ev float64 at the
 * 256-byte aligned offset, exactly the layout eks_fit writes for EKS_YEV64
 * (y is float64 whatever the members' type: an even m averages two members).
 * eks_smooth_gaps, eks_nll_sweep_gaps and eks_fit_gaps read them with
 * obs_dtype = EKS_YEV64.  nvalid (B T n bytes) or NULL: m of every column in
 * the planes' layout [t*n + j][b].
 * Limits: 1 <= n <= 64 and E <= eks_max_members(), else EKS_ERR_UNSUPPORTED.
 * EKS_ERR_ARG (before any launch): NULL obs / yev, T < 1, E < 1, a bad dtype
 * or mode, min_members outside [1, E].  B = 0: EKS_OK, nothing launched.
 * No workspace; results are bit-reproducible.
 */
int eks_ensemble_gaps(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n,
                      int64_t sb, int64_t st, int64_t se, int64_t sj, int mode, int min_members,
                      void *yev, uint8_t *nvalid, void *stream);

/*
 * eks_fit_pupil -- the statistics of the pupil model (eks/pupil_smoother.py:
 * 109-172) on the device, for B trajectories at once: the mean and population
 * variance (ddof 0) of the pupil diameter and of the pupil centre over the
 * complete frames.
 *
 *   obs      member observations, strides as eks_ensemble (EKS_F32 / EKS_F64),
 *            columns in the order top x, y, bottom x, y, right x, y, left x, y;
 *            or y / ev hand-off planes for (B, T, 8) (EKS_YEV32 / EKS_YEV64, as
 *            eks_fit_gaps accepts: the strides, E and mode are then ignored and
 *            yev must be NULL)
 *   n        must be 8, else EKS_ERR_UNSUPPORTED; T >= 2; E <= eks_max_members()
 *   stats    (B, 6) float64: mean diameter, mean centre x, y, var diameter,
 *            var centre x, y
 *   ncomplete (B) int32, REQUIRED: the complete frames
 *   status   (B) int32, REQUIRED; zeroed by the call.  A trajectory without a
 *            complete frame: EKS_STATUS_SINGULAR, ncomplete 0, NaN stats (the
 *            other trajectories are unaffected); exactly one complete frame:
 *            variances exactly 0
 *   yev      NULL, or (member input only) eks_yev_bytes(B, T, 8, EKS_F64, E,
 *            mode) bytes: the ensemble planes, always EKS_YEV64, bit-identical
 *            to eks_ensemble_gaps(min_members = E) on the same members -- what
 *            eks_nll_sweep_gaps / eks_smooth_gaps read, so the members are read
 *            once for fit + sweep + smooth
 *
 * A frame is complete iff the ensemble average and variance of all 8 columns
 * are finite (eks_fit_gaps's rule); from members a column is missing under the
 * all-members rule, and a min_members rule comes in through the planes of
 * eks_ensemble_gaps.  Only complete frames enter the statistics: the
 * reference's nanmedian rescue of partly observed frames is deliberately not
 * reproduced (this is the host fit on preds[ok]).  Per complete frame the
 * diameter is the median of the six estimates (top-bottom, left-right, the
 * four neighbour pairs x sqrt 2), the centre the mean of the two pair
 * midpoints per coordinate.  No floating-point atomics: results are
 * bit-identical from run to run.
 * EKS_ERR_ARG before any launch: a NULL pointer, a bad dtype or mode, T < 2,
 * E < 1, a workspace below eks_fit_pupil_workspace_bytes (0 for B <= 0 or
 * T < 2).  B = 0: EKS_OK, nothing launched.
 */
size_t eks_fit_pupil_workspace_bytes(int64_t B, int64_t T);
int eks_fit_pupil(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n,
                  int64_t sb, int64_t st, int64_t se, int64_t sj, int mode, double *stats,
                  int32_t *ncomplete, void *workspace, size_t workspace_bytes, int32_t *status,
                  void *yev, void *stream);

/*
 * eks_interp1d -- linear resampling for the asynchronous two-camera paw
 * smoother (F4), replacing the scipy.interpolate.interp1d(kind='linear')
 * calls of eks/multiview_pca_smoother.py:86-96 (which delegate to np.interp
 * for 1-D float64 columns): out(q, c) = y interpolated at xq[q] for each of
 * the ncol columns of y (element (k, c) at y[k*sy_row + c*sy_col]), sample
 * times x (nx, ascending).  Bit-identical to np.interp.  status (nq) or NULL:
 * EKS_STATUS_BAD_MODEL for queries outside [x[0], x[nx-1]] (interp1d raises
 * there; the output is NaN).  Device pointers, f64.
 */
int eks_interp1d(const double *x, int64_t nx, const double *y, int64_t ncol, int64_t sy_row,
                 int64_t sy_col, const double *xq, int64_t nq, double *out, int64_t so_row,
                 int64_t so_col, int32_t *status, void *stream);

/*
 * Test and fault-injection settings (process-wide, not part of the
 * smoother's semantics; tests only).  Returns the previous value.
 *   EKS_DBG_WAIT_US        bound of every in-launch chain wait of the
 *                          time-parallel passes, in microseconds of wall-clock
 *                          time (0 = the default, 1 s).  A wait that reaches
 *                          it gives up, flags its trajectories EKS_STATUS_SCAN
 *                          and lets the launch finish.  -1 = every wait gives
 *                          up at once (drives the time-out path).
 *   EKS_DBG_A3_SLICE_BYTES largest member byte offset span of one algo-3
 *                          launch (0 = 4 GB, the buffer descriptor's range);
 *                          a smaller span forces the batch slicing.
 *   EKS_DBG_FIT_SELECT     eks_fit's percentile selection: 0 = automatic
 *                          (split over row segments for B < 512 rows), 1 =
 *                          one block per row, 2 = split (both must give the
 *                          same threshold and kept-frame mask).  The
 *                          workspace size follows the setting.
 *   EKS_DBG_A3_MODE        retired (round 5): algo 3 has one launch form,
 *                          the forward pass then the backward pass; the key
 *                          still round-trips its value and changes nothing.
 *   EKS_DBG_A3_LB          algo 3's backward look-back: 0 = automatic (batches
 *                          of at most 48 64-trajectory groups), 1 = never,
 *                          2 = always.  Results are bit-identical.
 *   EKS_DBG_RT_FORM        the runtime-n smoother (algo 4): 0 = automatic
 *                          (time-parallel when the trajectories alone do not
 *                          fill the GPU), 1 = one lane per trajectory, 2 =
 *                          time-parallel.  Results agree to rounding; set it
 *                          before eks_smooth_workspace_bytes.
 *   EKS_DBG_PVAR_CHUNK     eks_smooth_var's chunk length: 0 = automatic, else
 *                          that many steps rounded up to a multiple of 8
 *                          (>= T: one chunk).  Set it before
 *                          eks_smooth_var_workspace_bytes.
 *   EKS_DBG_SWEEP_CHUNK    eks_nll_sweep's chunk length, with the same rule.
 *                          Set it before eks_nll_sweep_workspace_bytes.
 *   EKS_DBG_GAPS_CHUNK     eks_smooth_gaps's chunk length, with the same rule.
 *                          Set it before eks_smooth_gaps_workspace_bytes.
 *   EKS_DBG_GAPS_SWEEP_CHUNK  eks_nll_sweep_gaps's chunk length, with the same
 *                          rule.  Set it before
 *                          eks_nll_sweep_gaps_workspace_bytes.
 *   EKS_DBG_DRAWS_RAW      non-zero: eks_draws_noise writes the generator's
 *                          53-bit integers (k1, k2 of each block, as doubles)
 *                          in place of the normals.  eks_draws_gaps ignores it.
 */
enum { EKS_DBG_WAIT_US = 1, EKS_DBG_A3_SLICE_BYTES = 2, EKS_DBG_FIT_SELECT = 3,
       EKS_DBG_A3_MODE = 4, EKS_DBG_A3_LB = 5, EKS_DBG_RT_FORM = 6, EKS_DBG_PVAR_CHUNK = 7,
       EKS_DBG_SWEEP_CHUNK = 8, EKS_DBG_GAPS_CHUNK = 9, EKS_DBG_GAPS_SWEEP_CHUNK = 10,
       EKS_DBG_DRAWS_RAW = 11 };
int64_t eks_debug_set(int key, int64_t value);

/*
 * Profiling aid (not part of the smoother's semantics).  After
 * eks_profile_begin(max_calls), each eks_smooth call on this thread records
 * a hipEvent on its stream before each of its kernels and after the last one
 * (at most max_calls calls).  eks_profile_end synchronises on those events,
 * writes the per-kernel average milliseconds over the recorded calls into
 * kernel_ms[0..k) and the kernel names into names[k * name_len] (host
 * buffers), switches profiling off and returns k (kernels per call).
 */
int eks_profile_begin(int max_calls);
int eks_profile_end(double *kernel_ms, char *names, int max_kernels, int name_len);

#ifdef __cplusplus
}
#endif
#endif /* EKS_HIP_H */
