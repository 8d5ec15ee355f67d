/*
 * iwvi_hip.h -- C-ABI of the MI355X (gfx950) importance-weighted-ELBO hot path.
 *
 * The reference (hughsalimbeni/DGPs_with_IWVI) has no FFI: its hot path is a
 * chain of TensorFlow-1/GPflow-1 ops behind Python class signatures.  Each entry
 * point below replaces the op group named in its comment (file:line relative to
 * the reference checkout); dgps_with_iwvi_amd/{temp_workaround,layers,models}.py
 * bind them with ctypes and keep the reference's Python signatures.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *     the caller (PyTorch-ROCm) owns every buffer; nothing is allocated here;
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered,
 *     there is no global mutable state except the thread-local error string,
 *     and no call synchronises the device (safe inside hipGraph capture);
 *   - return 0 on success, negative IWVI_ERR_* otherwise, text in iwvi_last_error();
 *   - dense row-major float32 tensors unless stated; "T" is the flattened sample
 *     batch (B*K rows of the reference's [B, K, D] tensors, or N rows of [N, D]).
 */
#ifndef IWVI_HIP_H
#define IWVI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 19, with additive extensions: iwvi_dgp_predict_samples and iwvi_sample_stats, then the iwvi_lik_* entry points (likelihoods other than
 * the Gaussian; iwvi_lik_predict_mixture, their Monte Carlo predictive mixture, last), were added without a change to any existing entry point or struct, so the number did not move and a caller built against
 * 19 keeps working; iwvi_sample_scores and iwvi_energy_score (proper scoring rules of predictive samples) and iwvi_psis_summary (importance-weight summaries with the Pareto-k diagnostic) likewise.  A C caller that wants the new symbols looks them up (dlsym), Python asks hasattr(lib, ...). */
#define IWVI_ABI_VERSION 19

enum {
    IWVI_OK = 0,
    IWVI_ERR_ARG = -1,      /* bad size / null pointer / unsupported combination */
    IWVI_ERR_LAUNCH = -2,   /* hip launch or runtime error (text has hipGetErrorString) */
    IWVI_ERR_UNSUPPORTED = -3
};

/* stationary kernels of gpflow.kernels used on the path (temp_workaround.py:39,44,45) */
enum { IWVI_KERN_RBF = 0, IWVI_KERN_MATERN52 = 1 };

/* Encoder(activation_func=...) (layers.py:109,119,143-144; the reference's default is tf.nn.tanh) */
enum { IWVI_ACT_TANH = 0, IWVI_ACT_RELU = 1, IWVI_ACT_SIGMOID = 2, IWVI_ACT_SOFTPLUS = 3, IWVI_ACT_IDENTITY = 4 };

/* gpflow.mean_functions used by GPLayer.propagate (layers.py:46-48) */
enum { IWVI_MF_ZERO = 0, IWVI_MF_IDENTITY = 1, IWVI_MF_LINEAR = 2 };

#define IWVI_MAX_LAYERS 8   /* GP layers batched into one precompute launch   */
#define IWVI_MAX_R 32       /* latent GPs per layer                            */
#define IWVI_MAX_P 32       /* mixed outputs per layer                         */
#define IWVI_MAX_D 32       /* layer input dimension                           */
#define IWVI_MAX_M 512      /* inducing points per layer                       */
#define IWVI_MAX_KL 4       /* local-regulariser arrays fed to the ELBO reduce */
#define IWVI_MAX_ENC 8      /* encoder MLP layers                              */

int iwvi_version(void);
const char* iwvi_last_error(void);

/* ------------------------------------------------------------------------
 * Per-step, per-GP-layer state ("the inducing-set factorisation").
 * Replaces: Kuu(feat, kern, jitter) + tf.cholesky  (temp_workaround.py:39,48),
 * the operand side of tf.matrix_triangular_solve (:51), tf.matrix_band_part of
 * q_sqrt (:78), the operand side of Kuf (:44) and gauss_kl (layers.py:44 ->
 * temp_workaround.py:186-188).
 *
 * Mp = M rounded up to 16, nbk = Mp/16, ntri = nbk(nbk+1)/2.  Packed operands are
 * 16x16 blocks in v_mfma_f32_16x16x4_f32 fragment order.
 * The state buffer holds, in this order,
 *   double  Lm   [Mp*Mp]   lower Cholesky factor of Kuu   (written only with IWVI_GP_WANT_DENSE)
 *   double  Linv [Mp*Mp]   Lm^-1                          (written only with IWVI_GP_WANT_DENSE)
 *   float   LsP  [ntri*256]        forward-substitution stream of matrix_triangular_solve (:51): row-block bi =
 *                                  [-Lm(bi,0) .. -Lm(bi,bi-1), Lm(bi,bi)^-1], packed.  Layers with an even nbk <= 8 hold
 *                                  the off-diagonal blocks as split-f16 halves (16 B per lane: h1 x 4 | h2 x 4 of
 *                                  2^est (-Lm(bi,bj))) and the inverse diagonal blocks times 2^(-2 est): the state is an
 *                                  opaque operand image of the fused kernels, not an interchange format
 *   float   LrTP [R*ntri*256]      tril(q_sqrt[r])^T, upper-triangular blocks, packed
 *   float   QmuP [ceil(R/16)*nbk*256]  q_mu^T, packed  (mean = A^T q_mu, :68)
 *   float   ZtP  [nbk*9*64]        K_uf operand: augmented, centred, scaled inducing inputs
 *   float   cst  [64]              1 / lengthscales [32] | centre of Z / lengthscales [32]  (0 beyond D)
 *   double  kl   [IWVI_MAX_R]      kl[r] = latent GP r's share of the whitened KL[q(u) || p(u)]
 *                                  (the layer's KL is the sum of the first R entries)
 *   double  ws   [...]             factorisation workspace (16x16 blocks of the lower triangle)
 * iwvi_gp_state_bytes() returns the size; offsets via iwvi_gp_state_offsets().
 * ---------------------------------------------------------------------- */
#define IWVI_GP_WANT_DENSE 1   /* iwvi_gp_desc.flags: also write the dense float64 Lm and Lm^-1 */
#define IWVI_GP_WANT_LM    2   /* iwvi_gp_desc.flags: also write the dense float64 Lm (Lm^-1 then by iwvi_gp_dense_inverse)  */
/* iwvi_gp_desc.flags: prepare the layer for the float64 stage-1 route of the forward (IWVI_LAYER_F64_STAGE1 below): the precompute call
 * also leaves the dense float64 Lm and Lm^-1 (as with IWVI_GP_WANT_LM + iwvi_gp_dense_inverse, launched behind it on the same stream)
 * and the plain float32 inducing inputs z~ the factorisation saw. */
#define IWVI_GP_F64_STAGE1 4
/* iwvi_gp_desc.flags (ABI 17), for callers that KNOW which inputs moved since the last full precompute on this state buffer -- a
 * training step whose first op moves only the final layer's q(u) (build_models.py:288-300):
 * IWVI_GP_REUSE_FACTOR: Z, lengthscales, variance, jitter are unchanged: the factorisation and everything derived from it stay as they
 *   are, only the q(u) images (tril(q_sqrt)^T, q_mu^T, their split-f16 slabs and scales, kl[]) are rewritten -- ~5 us instead of ~26 at
 *   M = 128.  A layer of which nothing moved is simply left out of the call.
 * IWVI_GP_FACTOR_ONLY: the opposite -- the factorisation and its images only; the q(u) images are not touched (q may be written by
 *   another stream meanwhile).  Both together: error. */
#define IWVI_GP_REUSE_FACTOR 8
#define IWVI_GP_FACTOR_ONLY 16

typedef struct iwvi_gp_desc {
    const float* Z;            /* [M, D]  inducing inputs                        */
    const float* lengthscales; /* [D]     ARD lengthscales                       */
    const float* q_mu;         /* [M, R]                                         */
    const float* q_sqrt;       /* [R, M, M]; only the lower triangle is read     */
    void* state;               /* iwvi_gp_state_bytes(M, R) bytes, 256-B aligned */
    float variance;            /* kernel variance sigma^2                        */
    double jitter;             /* gpflow settings.numerics.jitter_level          */
    int32_t M, D, R;
    int32_t kern_type;         /* IWVI_KERN_*                                    */
    int32_t flags;             /* IWVI_GP_* bits above, or 0                     */
    const float* variance_dev; /* optional DEVICE scalar: read instead of `variance` when the launch runs (a trained
                                * kernel variance that lives on the device keeps a captured hipGraph valid across steps) */
} iwvi_gp_desc;

size_t iwvi_gp_state_bytes(int M, int R);
/* offsets (bytes) of {Lm, Linv, LsP, LrTP, QmuP, ZtP, cst, kl} inside the state buffer */
int iwvi_gp_state_offsets(int M, int R, size_t out_host[8]);

/* factorise up to IWVI_MAX_LAYERS layers per launch: grid (layer, role) -- role 0 Gram + Cholesky +
 * triangular inverse + packing, roles 1..R tril(q_sqrt[r])^T packing + KL share */
int iwvi_gp_precompute(const iwvi_gp_desc* layers_host, int n_layers, void* stream);
/* Lm^-1 (dense float64) from the dense Lm of states precomputed with IWVI_GP_WANT_LM (or _DENSE): one workgroup per 16-column block of
 * the inverse, n_layers <= IWVI_MAX_STACK in one launch.  The adjoint's route to the dense factors: one factorisation serves the
 * forward and the backward, and the inversion does not sit on the factorising workgroup's CU. */
int iwvi_gp_dense_inverse(const iwvi_gp_desc* layers_host, int n_layers, void* stream);

/* The same launch can also evaluate the Encoder MLP of a LatentVariableLayer (layers.py:137-152) for every row of
 * the minibatch: it does not depend on the factorisation, so it runs on otherwise idle CUs, off the critical
 * path of iwvi_dgp_forward (which then takes iwvi_layer_desc.enc_out instead of the weights).
 *   XY [rows, dims[0]];  enc_W[i] [dims[i], dims[i+1]], enc_b[i] [dims[i+1]] (host arrays of device pointers);
 *   out [rows, 2*latent_dim] = (means | raw), q_sqrt = softplus(raw - 3).
 * An encoder role keeps its weights, biases and two 256-row activation buffers in LDS: (w + 4 + 2 * 256 * 65) floats for w weights and
 * biases, so w <= 7676 (e.g. widths [64, 64, 64, 2] do not fit).  A larger encoder is refused with IWVI_ERR_UNSUPPORTED before
 * anything is launched; iwvi_dgp_forward evaluates it from iwvi_layer_desc.enc_W. */
typedef struct iwvi_enc_desc {
    const float* XY; int64_t rows;
    const float* const* enc_W; const float* const* enc_b; const int32_t* dims; int32_t n_enc, latent_dim;
    float* out;
    /* optional sampling tail (sample_X == NULL: absent).  For the IW tiling -- K samples per data row, sample
     * t = row * K + k -- the whole LatentVariableLayer is evaluated here instead of in the layer kernel (it needs
     * nothing from the factorisation): W = q_mu + z softplus(raw - 3) (layers.py:83-87), with z drawn from the same
     * counter-based stream the layer kernel would use for layer `layer_index` of evaluation *rng_state. */
    const float* X; int32_t Dx;          /* data rows [rows, Dx] (the minibatch, untiled) */
    int32_t K, sampled_kl, layer_index;
    uint64_t seed; const uint64_t* rng_state;
    float* sample_X;                     /* [rows * K, Dx + latent_dim] = concat(X tiled, W)          (layers.py:89) */
    float* sample_kl;                    /* [rows * K] local regulariser summed over the latent dims  (:98-103)      */
    float* sample_z;                     /* optional [rows * K, latent_dim]: the draws                               */
    int32_t act;                         /* IWVI_ACT_* of the hidden layers (0 = tanh)                                */
} iwvi_enc_desc;
int iwvi_model_precompute(const iwvi_gp_desc* layers_host, int n_layers,
                          const iwvi_enc_desc* encs_host, int n_encs, void* stream);

/* K1: Kuu(feat, kern, jitter) in float64 (temp_workaround.py:39)  -> Kuu [M, M] double */
int iwvi_rbf_gram_sym(const float* Z, const float* lengthscales, float variance, double jitter,
                      int kern_type, int M, int D, double* Kuu, void* stream);
/* K2: tf.cholesky(Kmm) in float64 (temp_workaround.py:48): A [M, M] (lower triangle read) ->
 * Lout [M, M] lower factor (upper triangle zero); ws = iwvi_chol_ws_bytes(M) bytes of scratch */
size_t iwvi_chol_ws_bytes(int M);
int iwvi_chol_factor(const double* A, double* Lout, int M, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * GPLayer forward on a flattened sample batch (diag / marginal variance).
 * Replaces: Kuf (:44), matrix_triangular_solve (:51), Kdiag - sum A^2 (:59),
 * A^T q_mu (:68), einsum('rMm,sMn->srmn') (:78), + sum LTA^2 (:85), the
 * marginal sample (:89-91), SharedMixedMok mixing (:142-145) and the mean
 * function add (layers.py:46-48) -- one fused launch, nothing spilled to HBM.
 *
 *   F      [T/bcast_K, D]  layer input; bcast_K >= 1: every row stands for bcast_K consecutive samples
 *                   (the tiling of models.py:113 done inside the kernel); 1 = F has T rows
 *   noise  [T, R]   N(0,1) draws (z of temp_workaround.py:89); may be NULL -> z = 0
 *   W      [P, R]   SharedMixedMok.W, or NULL (then P must equal R)
 *   mf_A   [D, P], mf_b [P]  for IWVI_MF_LINEAR (mf_b may be NULL)
 *   sample/mean/var [T, P]   any may be NULL (not written)
 * var is clamped at 0 (float32 cancellation can undershoot; the reference is fp64).
 * ---------------------------------------------------------------------- */
int iwvi_gp_layer_forward(const void* state, int M, int D, int R, int P,
                          int kern_type, float variance,
                          const float* F, const float* noise, const float* W,
                          int mf_type, const float* mf_A, const float* mf_b,
                          float* sample, float* mean, float* var,
                          int64_t T, int bcast_K, void* stream);
/* the same with iwvi_layer_desc.flags bits for the layer (IWVI_LAYER_F32_STAGE2, IWVI_LAYER_F64_STAGE1); the plain entry = flags 0 */
int iwvi_gp_layer_forward_ex(const void* state, int M, int D, int R, int P,
                             int kern_type, float variance,
                             const float* F, const float* noise, const float* W,
                             int mf_type, const float* mf_A, const float* mf_b,
                             float* sample, float* mean, float* var,
                             int64_t T, int bcast_K, int layer_flags, void* stream);

/* Full covariance over the second axis (temp_workaround.py:45,56,83 with full_cov=True):
 *   F [S, N, D] -> mean [S, N, R] (+ the layer's mean function, layers.py:46-48: mf_type / mf_A [D, R] / mf_b [R] as
 *   iwvi_gp_layer_forward), cov [S, R, N, N].
 * ws: iwvi_gp_fullcov_ws_bytes(S*N, M, R) bytes of scratch (A and LTA, as the reference
 * materialises them). Plain kernels only (the SharedMixedMok branch forces full_cov=False). */
size_t iwvi_gp_fullcov_ws_bytes(int64_t T, int M, int R);
int iwvi_gp_layer_fullcov(const void* state, int M, int D, int R, int kern_type, float variance,
                          const float* F, int64_t S, int64_t N,
                          int mf_type, const float* mf_A, const float* mf_b,
                          float* mean, float* cov, void* ws, void* stream);
/* the same with iwvi_layer_desc.flags bits.  IWVI_LAYER_F64_STAGE1: a = Lm^-1 k comes from the float64 route, and the covariance
 * k(x_i, x_j) - a_i . a_j + u_i . u_j is differenced and accumulated in float64 before it is rounded to the float32 output. */
int iwvi_gp_layer_fullcov_ex(const void* state, int M, int D, int R, int kern_type, float variance,
                             const float* F, int64_t S, int64_t N,
                             int mf_type, const float* mf_A, const float* mf_b,
                             float* mean, float* cov, void* ws, int layer_flags, void* stream);

/* The jointly Gaussian sample of the full-covariance branch (temp_workaround.py:93-96, with the intended
 * fmean_SRN1 of :95):  sample[s, n, r] = mean[s, n, r] + (chol(cov[s, r] + jitter I) z[s, r])[n].
 * mean, sample [S, N, R]; cov [S, R, N, N]; z [S, R, N].  N <= 192 (N is the importance-sample axis on the IW path)
 * factorises in LDS; larger N needs ws = iwvi_mvn_sample_ws_bytes(S, N, R) bytes of scratch (0 for N <= 192) and is
 * latency-bound.  Rounding-tolerant PSD factorisation: the block is a float32 difference k - a.a + u.u and (near-)singular
 * blocks (X tiled over K: rank 1) are indefinite by rounding, so a non-positive pivot zeroes its column instead of
 * failing like tf.cholesky, and entries are clamped to |L_ij| <= sqrt(C_ii); on a well-conditioned block this is chol(). */
size_t iwvi_mvn_sample_ws_bytes(int64_t S, int N, int R);
int iwvi_mvn_sample(const float* mean, const float* cov, const float* z, float* sample,
                    int64_t S, int N, int R, float jitter, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * The whole layer stack of DGP_VI.propagate (models.py:31-46) for a flattened sample batch in ONE
 * launch, ending in the per-sample log-weight of models.py:134-142.  Every sample's path through the
 * layers is independent of the other samples, so a workgroup keeps its chunk of samples in LDS from
 * the tiled input (models.py:113-116) to the Gaussian variational expectation (:134); only the
 * optional per-layer outputs and the log-weights [T] touch HBM.
 *
 * Row t of the batch stands for data row (t / row_div) % row_mod of X / XY / Y:
 *   IW tiling [B, K, .] (models.py:113-116): row_div = K, row_mod = B;  VI tiling tile(X, [S, 1])
 *   (:50-53): row_div = 1, row_mod = N;  an explicit [T, .] input: row_div = 1, row_mod = T.
 * layers[i].type selects GPLayer (layers.py:35-50; state from iwvi_gp_precompute) or
 * LatentVariableLayer (layers.py:72-105, encoder :137-152).  Per layer:
 *   noise      [T, R] (GP) / [T, latent_dim] (LV) N(0,1) draws, or NULL: drawn in-kernel from the
 *              counter-based stream (seed, step, layer, t) documented in DESIGN.md
 *   noise_out  optional: the draws that were used
 *   sample / mean / var   optional [T, P] (GP) or [T, D + latent_dim] (LV) outputs
 *   kl_local   LV only, optional [T, latent_dim]: log q(W) - log p(W) (sampled_kl) or the analytic KL
 * rng_state: 2 device words {step counter, ticket}, zeroed once by the caller; the launch reads the step
 *   and its last workgroup advances it, so a replayed hipGraph draws fresh noise.  May be NULL when every
 *   layer has explicit noise.  The ticket word is the launch's arrival counter (every workgroup adds to it once,
 *   the last one leaves it at 0): two launches that may overlap in time need their own rng_state.
 * Y / out_logw may be NULL (propagate only).  out_logw [T] = sum_d var_exp - sum local regularisers.
 * ---------------------------------------------------------------------- */
enum { IWVI_LAYER_GP = 0, IWVI_LAYER_LV = 1 };
#define IWVI_MAX_STACK 8    /* layers (GP + LV) in one fused launch */

typedef struct iwvi_layer_desc {
    int32_t type;                   /* IWVI_LAYER_*                                          */
    /* GP layer */
    const void* state;              /* precomputed iwvi_gp_desc.state                        */
    int32_t M, D, R, P;             /* inducing points, input dim, latent GPs, outputs       */
    int32_t kern_type, mf_type;     /* IWVI_KERN_*, IWVI_MF_*                                */
    float variance;
    const float* W;                 /* [P, R] SharedMixedMok.W or NULL (then P == R)         */
    const float* mf_A;              /* [D, P] for IWVI_MF_LINEAR                             */
    const float* mf_b;              /* [P] or NULL                                           */
    /* LV layer (D = input dim as above) */
    const float* const* enc_W;      /* host array of n_enc device pointers, or NULL = prior  */
    const float* const* enc_b;
    const int32_t* enc_dims;        /* host: n_enc + 1 widths, [0] = XY width, [n] = 2*latent */
    int32_t n_enc, latent_dim, sampled_kl;
    const float* enc_out;           /* [data rows, 2*latent_dim] from iwvi_model_precompute: used instead of enc_W    */
    /* both */
    const float* noise;             /* explicit N(0,1) draws, or NULL                        */
    int32_t zero_noise;             /* noise == NULL: 1 -> z = 0 (sample == mean), 0 -> draw in-kernel */
    float* noise_out;
    float* sample; float* mean; float* var;
    float* kl_local;
    float* a_out; float* u_out;     /* GP, optional (what the adjoint needs): A [T, Mp], L_r^T A [R, T, Mp] */
    float* gmv_out;                 /* GP, optional: [T, 3R] = (sample | mean | variance) of the R latent GPs before mixing */
    const float* variance_dev;      /* GP, optional device scalar read instead of `variance` (see iwvi_gp_desc) */
    int32_t enc_act;                /* LV: IWVI_ACT_* of the encoder's hidden layers (0 = tanh) */
    int32_t flags;                  /* GP: IWVI_LAYER_* bits below (0 = the default arithmetic) */
} iwvi_layer_desc;
/* Arithmetic of the R * M^2 contraction u_r = tril(q_sqrt_r)^T a (temp_workaround.py:78) and of mean = q_mu^T a (:68), per CALL
 * (no process-wide mode: two threads may differ).  Default: split-f16 operands (x = h1 + h2, three v_mfma_f32_16x16x32_f16 per slab,
 * fp32 accumulate, per-matrix power-of-two scales; 22 operand mantissa bits -- DESIGN.md section 4) whenever every GP layer of the
 * launch has an even number of 16-row blocks.  IWVI_LAYER_F32_STAGE2 on ANY GP layer of a launch makes the whole launch take the
 * fp32-MFMA variant (v_mfma_f32_16x16x4_f32). */
#define IWVI_LAYER_F32_STAGE2 1
/* iwvi_layer_desc.flags, per GP layer: K_uf, a = Lm^-1 k and sigma^2 - |a|^2 of THIS layer in float64 (v_mfma_f64_16x16x4_f64 against the
 * dense float64 Lm^-1; temp_workaround.py:44,51,59 -- the reference computes all of it in float64), a rounded to float32 only behind the
 * solve.  For ill-conditioned K_uu (many inducing points in a 1-3-dimensional box: cond(Lm) ~ 1e4, where a float32 k alone costs 5e-4 of
 * the mean and the float32 solve 1e-2 .. 1e-1) it brings the per-layer mean / variance to ~1e-6 of the float64 reference; it costs a
 * float64 Gram and M^2 float64 MFMA FLOPs per sample (half the fp32-MFMA rate), and the launch then runs stage 2 on fp32 MFMAs.
 * The layer's state must have been precomputed with IWVI_GP_F64_STAGE1. */
#define IWVI_LAYER_F64_STAGE1 2

/* Optional tail of the same launch: the last workgroup to finish performs models.py:138-150 on out_logw
 * (logsumexp over K minus log K, or the mean over S of :84; sum over points * scale; minus the global KLs),
 * so that one IW-ELBO evaluation is two launches (iwvi_gp_precompute + iwvi_dgp_forward).  Fields as the
 * arguments of iwvi_logw_reduce; needs rng_state (its second word is the arrival ticket). */
typedef struct iwvi_elbo_desc {
    int64_t B; int32_t K;
    int64_t stride_b, stride_k;
    const double* const* kl_global; const int32_t* kl_global_counts; int32_t n_glob;
    double scale; int32_t K_total, mode_vi;
    float* out_lse_ms; float* out_logp; double* out_elbo;
    double* ws;                     /* optional scratch, ceil(T/16) doubles, used when every point's K samples sit in one chunk (NULL -> the
                                     * last workgroup reads all of out_logw): one partial sum per workgroup; with out_elbo given and at
                                     * most 511 workgroups the partial sums travel in the workgroups' tickets instead (a 64-bit atomic on
                                     * rng_state[1]) and ws only holds, tagged with the evaluation's number, the partial sums too large
                                     * for that fixed-point field.  Contents are scratch either way */
    /* when the leading LatentVariableLayer was evaluated by iwvi_model_precompute (iwvi_enc_desc.sample_X): its local
     * regulariser per sample [T] (subtracted from the log-weights like models.py:141-142), and the position of this
     * stack's first layer in the model, so that its noise streams do not collide with that layer's; x_per_sample:
     * X is that layer's output [T, Dx], one row per sample (Y and XY keep the row_div / row_mod mapping). */
    const float* lw_init;
    int32_t noise_layer_base;
    int32_t x_per_sample;
    const float* lik_variance_dev;  /* optional device scalar read instead of iwvi_dgp_forward's lik_variance argument */
    /* Optional: the heads of the bound's adjoint from the same launch (what iwvi_iw_elbo_backward computes from the final layer's moments --
     * two launches less in front of the first layer adjoint of a value + gradient evaluation): adj_w [T] = d ELBO / d L_nk (scale x the
     * softmax over the K samples of models.py:146-148), adj_dmean / adj_dvar [T, Dy] = d ELBO / d final mean / variance, adj_sums [3] =
     * (sum_n (lse_n - log K), d ELBO / d lik_variance, the bound), written by the last workgroup.  All four or none.  Importance-weighted
     * bound only (mode_vi = 0), every point's K samples contiguous (stride_k = 1, stride_b = K) and inside one chunk of the launch
     * (K divides 16 x the launch's sub-tile count), ws given with room for two doubles per chunk, no K-sharded exchange (the weights of a
     * sharded job need the job-wide logsumexp: iwvi_iw_elbo_backward's lse_global).  Otherwise the call returns IWVI_ERR_UNSUPPORTED
     * before anything is launched -- fall back to iwvi_iw_elbo_backward. */
    float* adj_w; float* adj_dmean; float* adj_dvar; double* adj_sums;
} iwvi_elbo_desc;

int iwvi_dgp_forward(const iwvi_layer_desc* layers_host, int n_layers,
                     const float* X, int Dx, const float* XY, int XYdim, const float* Y, int Dy,
                     int64_t T, int64_t row_div, int64_t row_mod, float lik_variance,
                     uint64_t seed, uint64_t* rng_state, float* out_logw,
                     const iwvi_elbo_desc* elbo /* or NULL */, void* stream);

/* ----------------------------------------------------------------------
 * Backward pass (the reference gets these from TensorFlow's autodiff of the graph of
 * models.py:112-150, experiments/build_models.py:284-304).  Layer by layer; RBF and Matern-5/2 kernels.
 *
 * iwvi_gp_layer_backward: adjoint of iwvi_gp_layer_forward for T samples.
 *   state                  as precomputed WITH IWVI_GP_WANT_DENSE (the dense float64 Lm and Lm^-1 are read)
 *   F [T, D]               the layer's input rows (per sample)
 *   noise [T, R]           the draws the forward used (needed when d_sample is given)
 *   A [T, Mp], U [R, T, Mp]  a = Lm^-1 k and u_r = L_r^T a as the forward wrote them (a_out / u_out).  U may be NULL when
 *                          iwvi_gp_layer_backward_needs_u says 0 (M a multiple of 16 up to 512, T a multiple of 16 -- of 32 beyond
 *                          M = 256 --, the tiles within the LDS) and GMV is given: that shape takes the streaming
 *                          chain, which works from a alone (sum_r 2dv_r L_r u_r = sum_r 2dv_r (L_r L_r^T) a, dL_r = tril(G_r L_r))
 *   GMV [T, 3R]            optional, the forward's gmv_out
 *   d_sample/d_mean/d_var [T, P]  upstream gradients, any may be NULL (= 0)
 *   kl_weight              the objective contains -kl_weight * KL[q(u)||p(u)] of this layer (1 for the ELBO)
 *   outputs (any may be NULL): dF [T, D], dZ [M, D], dls [D], dvariance [1], dq_mu [M, R],
 *                          dq_sqrt [R, M, M] (lower triangle; zeros above), dW [P, R], dmf_A [D, P]
 *   ws                     iwvi_gp_layer_backward_ws_bytes(T, M, D, R) bytes
 * ---------------------------------------------------------------------- */
typedef struct iwvi_gp_bwd_desc {
    const void* state;
    const float* Z; const float* lengthscales; const float* q_mu; const float* q_sqrt;
    float variance;
    int32_t M, D, R, P, kern_type;
    const float* W; int32_t mf_type; const float* mf_A;
    const float* F; const float* noise; const float* A; const float* U;
    const float* GMV;               /* optional: the forward's gmv_out [T, 3R]; spares the adjoint a pass over A and U */
    const float* d_sample; const float* d_mean; const float* d_var;
    double kl_weight;
    float* dF; float* dZ; float* dls; float* dvariance; float* dq_mu; float* dq_sqrt;
    float* dW; float* dmf_A;        /* optional: [P, R] (SharedMixedMok.W), [D, P] (Linear mean function A) */
    void* side_stream;              /* optional hipStream_t: once dF is queued on `stream`, the parameter gradients of this
                                     * layer are queued there (after an event), so that they overlap the adjoint of the layer
                                     * below; the caller joins the two streams before reading the parameter gradients */
    void* side_stream2;             /* optional second side stream: the parameter branch then runs as two concurrent chains
                                     * (Cholesky adjoint | the other sums over samples); join both */
    int32_t prepared;               /* nonzero: iwvi_gp_layer_backward_prepare has already run on this (desc, ws) */
    const float* variance_dev;      /* optional device scalar read instead of `variance` (see iwvi_gp_desc) */
    int32_t phase;                  /* 0: the whole adjoint.  1: only the per-sample chain (dF and the partial sums are queued);
                                     * 2: only the parameter branch of a call made with phase 1 on the same descriptor and
                                     * workspace.  The caller orders 2 after 1 and may queue other work in between (so that, in a
                                     * captured graph, the next layer's chain follows this one's on the same hardware queue).
                                     * Shapes off the streaming chain do everything in phase 1; phase 2 is then a no-op. */
    int32_t flags;                  /* IWVI_BW_* bits below (0 = the default arithmetic) */
} iwvi_gp_bwd_desc;
/* IWVI_BW_F32_CHAIN: the adjoint chain's S_r products on fp32 MFMAs instead of split-f16 operands (per call, like IWVI_LAYER_F32_STAGE2). */
#define IWVI_BW_F32_CHAIN 1
/* IWVI_BW_OWN_QSCALE (ABI 17; read by the two prepare entries): the q(u) scales in the state's constant block may be stale -- the state
 * was last precomputed with IWVI_GP_FACTOR_ONLY, or q(u) has moved since --: take max |L_r| from q_sqrt itself (same value, same
 * rounding; +2 us of the launch).  The preparation then depends on the state's factorisation only, not on a precompute of the current q(u). */
#define IWVI_BW_OWN_QSCALE 4
/* (both sizing entries answer for either arithmetic mode a later call may select through desc.flags: the larger workspace; u is needed
 * when either mode's adjoint reads it) */
size_t iwvi_gp_layer_backward_ws_bytes(int64_t T, int M, int D, int R);
/* 1 if the adjoint of this layer shape takes the GEMM path (in either arithmetic mode) and therefore needs the forward's u_out, 0 if the
 * streaming chain (which works from a_out alone) will run */
int iwvi_gp_layer_backward_needs_u(int64_t T, int M, int D, int R, int P);
/* the parameter-only part of the adjoint (scaled inducing inputs, float32 Lm^-1, the streaming chain's packed operands
 * S_r = L_r L_r^T and Lm^-T): reads state (dense factors), Z, lengthscales, q_sqrt, M / D / R of the descriptor only, so it can
 * be queued on another stream beside the forward; then set desc.prepared.  Called implicitly otherwise. */
int iwvi_gp_layer_backward_prepare(const iwvi_gp_bwd_desc* desc, int64_t T, void* ws, void* stream);
/* The same for n layers (n <= IWVI_MAX_STACK) in ONE launch: descs[i] with its workspace ws[i]; every descriptor must ask for the same
 * arithmetic mode (flags & IWVI_BW_F32_CHAIN), else IWVI_ERR_ARG.  (The prepare steps of a model are queued beside the layer kernel,
 * which holds every CU; as separate launches they run one after the other once it retires.) */
int iwvi_gp_layers_backward_prepare(const iwvi_gp_bwd_desc* descs, int n, int64_t T, void* const* ws, void* stream);
/* Outputs left NULL are not formed.  With ONLY dq_mu / dq_sqrt given (what the natural-gradient op of build_models.py:288-295 reads)
 * the call reduces to the heads and the two sums over samples behind those gradients (on either path: the streaming chain, or the
 * GEMMs over a_out / u_out): no prepare step, no dense factors in `state`, no kernel adjoint, no adjoint of the factorisation; the
 * values are bit-identical to the full call's. */
int iwvi_gp_layer_backward(const iwvi_gp_bwd_desc* desc, int64_t T, void* ws, void* stream);

/* Adjoint of the ELBO tail (models.py:134-150) for the IW tiling (sample t = b*K + k):
 *   L_nk = sum_dy varexp(Y; fmean, fvar) - sum_i sum_q kl_local[i][t, q];  ELBO = scale * sum_n (lse_k L_nk - log K) - KL.
 * out_w [T] = d ELBO / d L_nk (scale * softmax over k), d_mean / d_var [T, Dy] = heads of the final layer,
 * out_sums[0] = sum_n (lse - log K), out_sums[1] = d ELBO / d lik_variance, out_sums[2] = the bound itself
 * (scale * out_sums[0] - the sum of the kl_global arrays, as iwvi_elbo_desc);  ws: 2*B doubles. Outputs may be NULL
 * except out_sums.  lse_global [B] (or NULL): K-sharded training -- the logsumexp of every point over ALL the job's
 * K_total samples (after the exchange of iwvi_lse_merge); the weights are then exp(L - lse_global), this rank's share of the
 * softmax, and out_sums[0] / [2] are the job's.  mode_vi != 0: the bound of DGP_VI (models.py:84: mean over the samples instead of the logsumexp). */
int iwvi_iw_elbo_backward(const float* fmean, const float* fvar, const float* Y, int Dy,
                          const float* const* kl_local, const int32_t* kl_dims, int n_local,
                          int64_t B, int K, float lik_variance, double scale, int mode_vi,
                          float* out_w, float* d_mean, float* d_var,
                          const double* const* kl_global, const int32_t* kl_global_counts, int n_glob,
                          const float* lse_global, int K_total,
                          double* out_sums, double* ws, void* stream);
/* the same with the likelihood variance read from device memory when the launch runs (lik_variance_dev != NULL) */
int iwvi_iw_elbo_backward_dev(const float* fmean, const float* fvar, const float* Y, int Dy,
                              const float* const* kl_local, const int32_t* kl_dims, int n_local,
                              int64_t B, int K, float lik_variance, const float* lik_variance_dev, double scale, int mode_vi,
                              float* out_w, float* d_mean, float* d_var,
                              const double* const* kl_global, const int32_t* kl_global_counts, int n_glob,
                              const float* lse_global, int K_total,
                              double* out_sums, double* ws, void* stream);

/* Adjoint of the LatentVariableLayer (layers.py:83-103): mu, sigma [B, latent_dim] (the encoder's outputs per data
 * row), noise [T, latent_dim] (the draws), dF_next [T, ld_next] = gradient w.r.t. the layer's output rows (columns
 * col0 .. col0+latent_dim-1 are W's; may be NULL), w [T] = d ELBO / d L_nk (the regulariser enters with -1; may be
 * NULL).  d_enc_out [B, 2*latent_dim] = gradient w.r.t. the encoder's (means | raw) output.  mu / sigma rows have stride
 * ld_enc; sigma_is_raw != 0: `sigma` holds the encoder's raw output (sigma = softplus(raw - 3)), so that the [B, 2*latent_dim]
 * block iwvi_model_precompute leaves can be passed as (out, out + latent_dim, 2*latent_dim, 1). */
int iwvi_lv_layer_backward(const float* mu, const float* sigma, int ld_enc, int sigma_is_raw, const float* noise,
                           const float* dF_next, int ld_next, int col0, const float* w,
                           int latent_dim, int64_t B, int K, int sampled_kl, float* d_enc_out, void* stream);

/* Adjoint of the Encoder MLP (layers.py:137-152): d_out [rows, dims[n_enc]] -> dW[i] [dims[i], dims[i+1]], db[i]. */
size_t iwvi_encoder_backward_ws_bytes(int64_t rows, const int32_t* dims, int n_enc);
int iwvi_encoder_backward(const float* XY, int64_t rows, const float* const* enc_W, const float* const* enc_b,
                          const int32_t* dims, int n_enc, const float* d_out,
                          float* const* dW, float* const* db, void* ws, void* stream);
/* the same for an encoder whose hidden layers use activation IWVI_ACT_* */
int iwvi_encoder_backward_act(const float* XY, int64_t rows, const float* const* enc_W, const float* const* enc_b,
                              const int32_t* dims, int n_enc, int act, const float* d_out,
                              float* const* dW, float* const* db, void* ws, void* stream);

/* iwvi_lv_layer_backward followed by iwvi_encoder_backward_act, as one launch plus the reduction (the training step's form: the
 * workgroup that back-propagates eight data rows through the encoder forms their d(means | raw) itself; same arithmetic, same sums).
 * dims[n_enc] must be 2 * latent_dim; XY [B, dims[0]]. */
int iwvi_lv_encoder_backward(const float* mu, const float* sigma, int ld_enc, int sigma_is_raw, const float* noise,
                             const float* dF_next, int ld_next, int col0, const float* w,
                             int latent_dim, int64_t B, int K, int sampled_kl,
                             const float* XY, const float* const* enc_W, const float* const* enc_b,
                             const int32_t* dims, int n_enc, int act,
                             float* const* dW, float* const* db, void* ws, void* stream);

/* The estimator of the encoder gradient (additive at ABI 19).  With e = noise[t, l], W = mu + e sigma, dfw = dF_next[t, col0 + l] (0 when
 * NULL) and w = w[t], the pathwise cotangent at the sample with the encoder parameters held fixed inside log q is
 *     T = dfw + w (e / sigma - W)                     (+w e / sigma: the path through -log q;  -w W: the path through log p(W))
 *   IWVI_LV_GRAD_IWAE  d mu += dfw - w W,       d sigma += (dfw - w W) e + w / sigma    (the reparameterised gradient of the bound)
 *   IWVI_LV_GRAD_DREG  d mu += (w / w_unit) T,  d sigma += (w / w_unit) T e             (doubly reparameterised, Tucker et al. 2019)
 *   IWVI_LV_GRAD_STL   d mu += T,               d sigma += T e                          ("sticking the landing", Roeder et al. 2017: biased for K > 1)
 * then d raw = d sigma (1 - exp(-sigma)) as before.  w_unit = the weight a point's samples share (the `scale` of iwvi_iw_elbo_backward,
 * num_data / B), so that w / w_unit is the normalised importance weight -- under K-sharding this rank's share of it, as w already is.
 * The estimator is uniform over the launch.  IWVI_ERR_ARG before any device work: an estimator outside 0..2; DREG / STL with
 * sampled_kl == 0 (the analytic regulariser has no such estimator) or with w == NULL; w_unit not finite or <= 0.
 * iwvi_lv_layer_backward / iwvi_lv_encoder_backward are these with (IWVI_LV_GRAD_IWAE, 1.0). */
enum { IWVI_LV_GRAD_IWAE = 0, IWVI_LV_GRAD_DREG = 1, IWVI_LV_GRAD_STL = 2 };
int iwvi_lv_layer_backward_ex(const float* mu, const float* sigma, int ld_enc, int sigma_is_raw, const float* noise,
                              const float* dF_next, int ld_next, int col0, const float* w,
                              int latent_dim, int64_t B, int K, int sampled_kl, int estimator, double w_unit,
                              float* d_enc_out, void* stream);
int iwvi_lv_encoder_backward_ex(const float* mu, const float* sigma, int ld_enc, int sigma_is_raw, const float* noise,
                                const float* dF_next, int ld_next, int col0, const float* w,
                                int latent_dim, int64_t B, int K, int sampled_kl, int estimator, double w_unit,
                                const float* XY, const float* const* enc_W, const float* const* enc_b,
                                const int32_t* dims, int n_enc, int act,
                                float* const* dW, float* const* db, void* ws, void* stream);

/* Running moments of a set of float32 tensors (the gradient signal-to-noise monitor): ONE Welford update of every tensor of the table,
 * in float64, in one launch:  c = *count_dev + 1;  d = x - mean;  mean += d / c;  m2 += d (x - mean);  then *count_dev = c (a one-thread
 * launch behind it, as iwvi_adam_step_dev advances its step count: a captured graph stays valid from replay to replay).
 * mean / m2 [n] start at zero with *count_dev = 0; the unbiased variance is m2 / (count - 1).  At most 48 tensors per call (the table is
 * passed like iwvi_adam_step's); n == 0 entries are skipped.  IWVI_ERR_ARG: a null pointer, n_tensors <= 0 or beyond 48, n < 0. */
typedef struct iwvi_moments_tensor { const float* x; double* mean; double* m2; int64_t n; } iwvi_moments_tensor;
int iwvi_moments_update(const iwvi_moments_tensor* tensors_host, int n_tensors, int64_t* count_dev, void* stream);

/* Test log-likelihood of experiments/run_conditional_density_estimation.py:148-169, batched over the test points:
 * samples: S predictive draws per point (element (s, n) at samples[s*sample_stride + n*point_stride]); y [N].
 * Gaussian KDE with Silverman's bandwidth 1.06 std S^(-1/5) (:158-162) -> out_logp [N]; squared error of the
 * sample mean (:165) -> out_sqerr [N]; optional out_mean_std [N, 2].  Outputs may be NULL. */
int iwvi_kde_loglik(const float* samples, int64_t sample_stride, int64_t point_stride, const float* y,
                    int64_t N, int S, float* out_logp, float* out_sqerr, float* out_mean_std, void* stream);

/* Optimiser steps of experiments/build_models.py:284-304.
 * iwvi_natgrad_step: GPflow NatGradOptimizer (natural parameterisation) on a whitened (q_mu [M, R], q_sqrt [R, M, M]),
 * in place, float64 inside; dq_mu / dq_sqrt = gradients of the ELBO (the objective that is maximised).
 * iwvi_adam_step: TensorFlow AdamOptimizer on GPflow's unconstrained variables; transform 0 = identity,
 * 1 = positive (param = softplus(x) + 1e-6), | IWVI_ADAM_GRAD_F64: `grad` points to doubles (the likelihood-variance
 * gradient leaves iwvi_iw_elbo_backward in float64); x/m/v are the optimiser's state (same length as param);
 * init != 0 fills them from the current parameter values instead of stepping; t = 1-based step count.
 * Precision of the positive transform: x is the master copy.  A step reads x, m, v and grad, forms d param / d x = sigmoid(x) from x, and
 * WRITES param = softplus(x) + 1e-6 (it never reads param), so a parameter near the 1e-6 floor moves as accurately as one of order 1:
 * x within a few float32 spacings of a float64 Adam per step, param within that times param.  beta1 / beta2 / eps are used as floats, in the
 * recurrences and in the bias correction of both entry points alike.  Rule and measurements: tests/adam_reference.py, DESIGN.md section 2. */
size_t iwvi_natgrad_ws_bytes(int M);
int iwvi_natgrad_step(float* q_mu, float* q_sqrt, const float* dq_mu, const float* dq_sqrt,
                      int M, int R, double gamma, void* ws, void* stream);
/* ABI 16: the same with the workspace sized for R latent GPs.  M <= 128: the step runs as five launches spread over the chip (their block
 * images take ~340 KB per latent GP at M = 128) when `ws_bytes` holds them for all R and R <= 8 (the spread route's inverse images hold 8
 * latent GPs), else -- as iwvi_natgrad_step does beyond the R its R-independent size happens to cover -- as one workgroup per latent GP: the
 * same result, ~1.7x the time.  iwvi_natgrad_ws_bytes_ex(M, R) is the size that takes the spread route whenever R <= 8; at R > 8 the step is
 * one workgroup per latent GP whatever the workspace.  iwvi_debug_last_natgrad_route(): 0 = multi-launch (M > 128), 1 = one workgroup per
 * latent GP, 2 = spread. */
size_t iwvi_natgrad_ws_bytes_ex(int M, int R);
int iwvi_natgrad_step_ex(float* q_mu, float* q_sqrt, const float* dq_mu, const float* dq_sqrt,
                         int M, int R, double gamma, void* ws, size_t ws_bytes, void* stream);
int iwvi_debug_last_natgrad_route(void);
#define IWVI_ADAM_GRAD_F64 16
typedef struct iwvi_adam_tensor {
    float* param; const float* grad; float* x; float* m; float* v; int64_t n; int32_t transform;
} iwvi_adam_tensor;
int iwvi_adam_step(const iwvi_adam_tensor* tensors_host, int n_tensors, double lr, double beta1, double beta2,
                   double eps, int64_t t, int maximise, int init, void* stream);
/* the same with the step count on the device: the launch uses *t_dev + 1 and then stores it back (one tiny extra launch),
 * so a captured hipGraph of a training step stays valid from step to step */
int iwvi_adam_step_dev(const iwvi_adam_tensor* tensors_host, int n_tensors, double lr, double beta1, double beta2,
                       double eps, int64_t* t_dev, int maximise, void* stream);

/* models.py:138-150 on precomputed log-weights: logw row of (point b, sample k) = b*stride_b + k*stride_k;
 * arguments as iwvi_iw_elbo_reduce. */
int iwvi_logw_reduce(const float* logw, int64_t B, int K, int64_t stride_b, int64_t stride_k,
                     const double* const* kl_global_host, const int32_t* kl_global_counts_host, int n_glob,
                     double scale, int K_total, int mode_vi,
                     float* out_lse_ms, float* out_logp, double* out_elbo, uint64_t* ticket, void* stream);

/* ------------------------------------------------------------------------
 * The bound family between the K-sample ELBO and the importance-weighted bound (csrc/bound_family.hip): MIWAE, CIWAE and the tempered
 * (VR-alpha / Renyi) bound as one triple.  groups G >= 1 divides K, K_g = K / G, group g holds the contiguous samples g K_g .. (g+1) K_g - 1
 * of the IW tiling; 0 < tau <= 1 (tau = 1 - alpha); 0 <= beta <= 1.  Per data point n:
 *   bound_n = beta (1/K) sum_k L_nk + (1 - beta) (1/G) sum_g (1/tau) [ logsumexp_{k in g}(tau L_nk) - log K_g ]
 *   w_nk    = d bound_n / d L_nk = beta / K + (1 - beta) / G softmax_{k' in group(k)}(tau L_nk')_k            (sum_k w_nk = 1)
 * (1, 1, 0) is the importance-weighted bound, beta = 1 the mean over the samples (iwvi_logw_reduce with mode_vi).  Both entries return
 * IWVI_ERR_ARG before any device work for a NULL descriptor, groups < 1 or K % groups != 0, tau outside (0, 1] or NaN, beta outside [0, 1]
 * or NaN, and for what iwvi_logw_reduce / iwvi_iw_elbo_backward_dev refuse.  No float atomics: two calls give the same bits.
 * ---------------------------------------------------------------------- */
typedef struct iwvi_bound_desc { int32_t groups; float tau; float beta; } iwvi_bound_desc;

/* On precomputed log-weights (row of (point b, sample k) = b*stride_b + k*stride_k), one launch.  Outputs, each may be NULL: out_logp [B] =
 * bound_n; out_ess [B] = Kish's effective sample size (sum_k e^(L - m))^2 / sum_k e^(2 (L - m)) of the point's importance weights over ALL K
 * samples, in [1, K], whatever the triple; out_elbo [1] = scale * sum_n bound_n - the sum of the kl_global arrays, which needs out_logp (the
 * workgroups publish through it) and a zero-initialised ticket word, re-zeroed by the last workgroup (as iwvi_iw_elbo_reduce). */
int iwvi_bound_logw_reduce(const iwvi_bound_desc* bound, const float* logw, int64_t B, int K, int64_t stride_b, int64_t stride_k,
                           const double* const* kl_global_host, const int32_t* kl_global_counts_host, int n_glob, double scale,
                           float* out_logp, float* out_ess, double* out_elbo, uint64_t* ticket, void* stream);

/* The heads of the adjoint under the triple, Gaussian likelihood, IW tiling (t = b*K + k): the arguments of iwvi_iw_elbo_backward_dev
 * without mode_vi, lse_global and K_total.  out_w [T] = scale * w_nk, d_mean / d_var [T, Dy] (any of the three may be NULL), out_sums[0] =
 * sum_n bound_n, out_sums[1] = d bound / d lik_variance, out_sums[2] = the bound; ws: 2*B doubles. */
int iwvi_bound_elbo_backward(const iwvi_bound_desc* bound, const float* fmean, const float* fvar, const float* Y, int Dy,
                             const float* const* kl_local, const int32_t* kl_dims, int n_local,
                             int64_t B, int K, float lik_variance, const float* lik_variance_dev, double scale,
                             float* out_w, float* d_mean, float* d_var,
                             const double* const* kl_global, const int32_t* kl_global_counts, int n_glob,
                             double* out_sums, double* ws, void* stream);

/* ------------------------------------------------------------------------
 * LatentVariableLayer forward alone (layers.py:72-105) with its Encoder MLP (:137-152).
 *   F   [T, D];  XY [T, XYdim] or NULL (prior mode, :73-81);  noise [T, Lw] or NULL (z = 0)
 *   enc_W[i] [dims[i], dims[i+1]], enc_b[i] [dims[i+1]], dims_host[n_enc+1],
 *   dims[0] = XYdim, dims[n_enc] = 2*Lw; tanh on all but the last layer, skip
 *   connection where dims[i] == dims[i+1]; q_sqrt = softplus(raw - 3).
 *   sample/mean/cov [T, D+Lw] (any may be NULL), kl [T, Lw]:
 *   sampled_kl != 0 -> log q(W) - log p(W) (:98-100) else analytic KL (:101-103).
 * (The IW path runs this layer inside iwvi_dgp_forward, once per data point.)
 * ---------------------------------------------------------------------- */
int iwvi_lv_layer_forward(const float* F, const float* XY, const float* noise,
                          const float* const* enc_W_host, const float* const* enc_b_host,
                          const int32_t* dims_host, int n_enc,
                          int D, int Lw, int sampled_kl,
                          float* sample, float* mean, float* cov, float* kl,
                          int64_t T, void* stream);
/* the same for an encoder whose hidden layers use activation IWVI_ACT_* (Encoder(activation_func=...), layers.py:109) */
int iwvi_lv_layer_forward_act(const float* F, const float* XY, const float* noise,
                              const float* const* enc_W_host, const float* const* enc_b_host,
                              const int32_t* dims_host, int n_enc, int act,
                              int D, int Lw, int sampled_kl,
                              float* sample, float* mean, float* cov, float* kl,
                              int64_t T, void* stream);

/* ------------------------------------------------------------------------
 * The IW-ELBO reduction (models.py:133-150): Gaussian variational expectations
 * (:134), sum over Dy (:138), minus local regularisers (:140-142), logsumexp over
 * K minus log K (:148), sum over points * scale minus global KLs (:150).
 *   fmean, fvar: Dy-wide rows, row of (point b, sample k) = b*stride_b + k*stride_k
 *                (IW tiling [B,K,Dy]: stride_b = K, stride_k = 1; VI tiling [S*N,Dy]: 1, N);
 *                fvar = diagonal variances;  Y [B, Dy]
 *   kl_local[i] rows of kl_dims[i] floats, same row indexing, for i < n_kl
 *   kl_global[i]: pointer to kl_global_counts[i] doubles (state.kl of GP layer i: its R KL shares;
 *                 counts NULL -> 1 each), n_glob of them
 *   out_lse_ms [B, 2] = (max_k L, sum_k exp(L - max)) per point, for K-sharded merging
 *   out_logp   [B]     logsumexp - log(K_total)   (K_total = K when not sharded)
 *   out_elbo   [1] double = sum(logp) * scale - sum(kl_global)
 *   ticket     [1] device word, zeroed ONCE by the caller (never per call): the last workgroup to finish
 *              performs the final sum and re-zeroes it, so the whole reduction is one launch; needed when
 *              out_elbo != NULL
 * Any out pointer may be NULL.  mode_vi != 0 -> reduce_mean over K instead (models.py:84).
 * ---------------------------------------------------------------------- */
int iwvi_iw_elbo_reduce(const float* fmean, const float* fvar, const float* Y,
                        float lik_variance, int64_t B, int K, int Dy,
                        int64_t stride_b, int64_t stride_k,
                        const float* const* kl_local_host, const int32_t* kl_dims_host, int n_kl,
                        const double* const* kl_global_host, const int32_t* kl_global_counts_host, int n_glob,
                        double scale, int K_total, int mode_vi,
                        float* out_lse_ms, float* out_logp, double* out_elbo, uint64_t* ticket, void* stream);

/* ABI 16: the same with the likelihood variance read from a 1-element device tensor when `lik_variance_dev` is not NULL (a TRAINED
 * likelihood variance lives on the device: a captured graph of a K-sharded training step stays valid while it changes, and no
 * device-to-host copy sits in the step); `lik_variance` is then only validated (> 0). */
int iwvi_iw_elbo_reduce_dev(const float* fmean, const float* fvar, const float* Y,
                            float lik_variance, const float* lik_variance_dev, int64_t B, int K, int Dy,
                            int64_t stride_b, int64_t stride_k,
                            const float* const* kl_local_host, const int32_t* kl_dims_host, int n_kl,
                            const double* const* kl_global_host, const int32_t* kl_global_counts_host, int n_glob,
                            double scale, int K_total, int mode_vi,
                            float* out_lse_ms, float* out_logp, double* out_elbo, uint64_t* ticket, void* stream);

/* Merge K-sharded partials after the RCCL exchange (not in the reference):
 *   ms_all [G, B, 2] gathered (max, sumexp) pairs -> logp [B], elbo [1] as above. */
int iwvi_lse_merge(const float* ms_all, int G, int64_t B, int K_total,
                   const double* const* kl_global_host, const int32_t* kl_global_counts_host, int n_glob,
                   double scale, float* out_logp, double* out_elbo, void* stream);

/* The same for n_steps independent evaluations exchanged in ONE all-gather (forward-only evaluation loops amortise
 * the latency-bound collective this way): ms_all [G, n_steps, B, 2] -> logp [n_steps, B] (or NULL), elbo [n_steps]. */
int iwvi_lse_merge_steps(const float* ms_all, int G, int n_steps, int64_t B, int K_total,
                         const double* const* kl_global_host, const int32_t* kl_global_counts_host, int n_glob,
                         double scale, float* out_logp, double* out_elbo, void* stream);

/* whitened gauss_kl alone (temp_workaround.py:186-188), K14: -> kl [1] double */
int iwvi_gauss_kl(const float* q_mu, const float* q_sqrt, int M, int R, double* kl, void* stream);

/* gpflow Gaussian.variational_expectations as a callable (the reference calls it on explicit moments,
 * models.py:66,134):  out[t, d] = -1/2 log 2pi - 1/2 log s2 - 1/2 ((Y[row(t), d] - Fmu[t, d])^2 + Fvar[t, d]) / s2,
 * row(t) = (t / row_div) % row_mod (the tilings of iwvi_dgp_forward; Y already tiled: row_div = 1, row_mod = T).
 * Fmu, Fvar, out [T, Dy].  (The hot path never calls this: the expectation is fused into iwvi_dgp_forward's tail.) */
int iwvi_gaussian_var_exp(const float* Fmu, const float* Fvar, const float* Y, float lik_variance,
                          int64_t T, int Dy, int64_t row_div, int64_t row_mod, float* out, void* stream);

/* gpflow 1.x Gaussian.predict_density / Gaussian.logp as one callable:
 *   out[t, d] = -1/2 log 2pi - 1/2 log s - 1/2 (Y[row(t), d] - Fmu[t, d])^2 / s,  s = Fvar[t, d] + variance  (Fvar == NULL: s = variance, logp)
 * with row(t) as in iwvi_gaussian_var_exp; variance = *lik_variance_dev when that device scalar is given, else lik_variance.  Fmu, Fvar, out [T, Dy]. */
int iwvi_gaussian_log_density(const float* Fmu, const float* Fvar, const float* Y, float lik_variance, const float* lik_variance_dev,
                              int64_t T, int Dy, int64_t row_div, int64_t row_mod, float* out, void* stream);

/* Monte Carlo log predictive density of the layer stack (ABI 19), the doubly-stochastic DGP's predict_density(X, Y, S):
 *   out_logp[n] = log (1/S) sum_s prod_d N(Y[n, d]; m_snd, v_snd + variance)
 * where (m_snd, v_snd) are the final layer's marginal moments of draw s through the inner layers (marginal samples, latent-variable
 * layers in prior mode: their enc_W / enc_out must be NULL).  One iwvi_dgp_forward launch over the N x S rows t = n S + s (row_div = S:
 * layer noise, injected or drawn, is indexed by that row) with a predictive tail -- no per-layer output, no per-sample log-weight reaches
 * memory -- and one small launch that merges each point's per-workgroup (max, sum exp) partials in a fixed order (deterministic).
 * X [N, Dx], Y [N, Dy] (Dy = the final layer's P), ws: iwvi_dgp_predict_density_ws_bytes(N, S) bytes of device memory, no initial
 * contents.  variance = *lik_variance_dev when given.  rng_state as in iwvi_dgp_forward (its step word advances once per call).
 * N x S < 2^31 - 4096. */
size_t iwvi_dgp_predict_density_ws_bytes(int64_t N, int64_t S);
int iwvi_dgp_predict_density(const iwvi_layer_desc* layers_host, int n_layers, const float* X, int Dx, const float* Y, int Dy,
                             int64_t N, int64_t S, float lik_variance, const float* lik_variance_dev, uint64_t seed,
                             uint64_t* rng_state, float* out_logp, void* ws, void* stream);

/* Predictive samples of y from the layer stack (additive extension of ABI 19), the doubly-stochastic DGP's predict_y_samples(X, S)
 * (reference models.py:104-107):
 *   out_y[n, s, d] = m_snd + sqrt(v_snd + variance) eps_snd
 * with (m_snd, v_snd) and the rows t = n S + s exactly as in iwvi_dgp_predict_density: ONE iwvi_dgp_forward launch whose tail writes the
 * samples -- no per-layer output reaches memory.  eps = z_y[t, d] ([N S, Dy]) when z_y is given; otherwise drawn from the launch's
 * counter-based stream under an index no layer uses, so the layers' own draws are those of the same call without the tail.
 * X [N, Dx]; out_y [N, S, Dy] (a point's S samples are contiguous: what iwvi_sample_stats reads fastest); Dy = the final layer's P;
 * variance = *lik_variance_dev when given.  rng_state as in iwvi_dgp_forward (its step word advances once per call); it may be NULL
 * only when z_y and every layer's noise are given.  N x S < 2^31 - 4096. */
int iwvi_dgp_predict_samples(const iwvi_layer_desc* layers_host, int n_layers, const float* X, int Dx, int Dy, int64_t N, int64_t S,
                             float lik_variance, const float* lik_variance_dev, const float* z_y, uint64_t seed,
                             uint64_t* rng_state, float* out_y, void* stream);

/* Per-point statistics of S samples in one launch (additive extension of ABI 19): the rest of the reference's evaluation loop
 * (experiments/run_conditional_density_estimation.py:148-169) and quantiles, from ONE ascending sort of each point's samples in LDS.
 * samples: element (s, n) at samples[s*sample_stride + n*point_stride] (positive strides), 2 <= S <= 16384; y [N].
 *   out_logp, out_sqerr, out_mean_std [N, 2]: as iwvi_kde_loglik (float64 sums); y may be NULL when neither out_logp nor out_sqerr is asked for
 *   out_W [N]: the Shapiro-Wilk statistic W = (sum_i a_i (x_(S+1-i) - x_(i)))^2 / sum_i (x_i - mean)^2 with Royston's coefficients
 *     (algorithm AS R94) a = sw_coef [S/2], float64 on the device; they depend on S alone and are computed by the caller (Python:
 *     evaluation.shapiro_coefficients).  All samples equal: W = 1.
 *   out_quantiles [N, n_probs]: at probs [n_probs] (device, float64 like NumPy's -- a float32 0.975 would move the position p (S - 1) by 4e-5 at
 *     S = 2000 --, each in [0, 1]; values outside are clamped), NumPy's default rule: position
 *     p (S - 1), linear interpolation between the two neighbouring sorted values.  n_probs = 0: none.
 * Every output may be NULL.  A point with a NaN sample gets NaN in all of its outputs; other points are not affected. */
int iwvi_sample_stats(const float* samples, int64_t sample_stride, int64_t point_stride, const float* y, int64_t N, int S,
                      const double* sw_coef, const double* probs, int n_probs, float* out_logp, float* out_sqerr,
                      float* out_mean_std, float* out_W, float* out_quantiles, void* stream);

/* Univariate proper scoring rules of S samples per point in one launch (additive extension of ABI 19; csrc/sample_scores.hip), from the
 * same ONE ascending sort x_(1) <= .. <= x_(S) as iwvi_sample_stats (csrc/sample_sort.h: one network, one grouping rule, one quantile rule).
 * samples, strides, S and N as iwvi_sample_stats; y [N] is required.  With
 *   A = (1/S) sum_s |x_s - y|,   G = sum_i (2i - S - 1) x_(i) = 1/2 sum_s sum_t |x_s - x_t|:
 *   out_crps [N, 2]: A - G / S^2, the ensemble CRPS (the CRPS of the samples' empirical distribution), and A - G / (S (S - 1)), the fair
 *     CRPS (unbiased for the CRPS of the distribution the samples were drawn from).  Valid for counts and labels as for reals.
 *   out_counts [N, 2] (int32): #{s : x_s < y} and #{s : x_s == y}, exact.  A PIT value / rank is formed from them by the caller, who
 *     decides what ties mean (mid-rank, or a uniform draw inside the tie for a discrete target).
 *   out_quantiles [N, n_probs]: at probs [n_probs] (device, float64, clamped to [0, 1]), NumPy's default linear rule: the arithmetic of
 *     iwvi_sample_stats, the same bits on the same input.  n_probs = 0: none.
 *   out_pinball [N, n_probs]: max(tau (y - Q), (tau - 1) (y - Q)), tau = probs[q], Q the float64 quantile before it is rounded.
 * Every sum is float64 formed from the float32 values, combined in a fixed order (no atomics: two calls give the same bits); each result
 * is rounded to float32 once.  Every output may be NULL.  A point with a NaN sample or a NaN y gets NaN in its float outputs and -1 in
 * both counts; other points are not affected.  N = 0: IWVI_OK without a launch.  IWVI_ERR_ARG before any HIP call for: S outside
 * 2 .. 16384, N outside 0 .. 2^31 - 1, null samples or y, a non-positive stride, n_probs < 0, n_probs > 0 without probs or without
 * either of out_quantiles / out_pinball. */
int iwvi_sample_scores(const float* samples, int64_t sample_stride, int64_t point_stride, const float* y, int64_t N, int S,
                       const double* probs, int n_probs, float* out_crps, int32_t* out_counts, float* out_quantiles,
                       float* out_pinball, void* stream);

/* The energy score, the multivariate CRPS, of S samples in D dimensions per point in one launch (additive extension of ABI 19;
 * csrc/energy_score.hip).  samples: coordinate d of sample s of point n at samples[s*sample_stride + n*point_stride + d*dim_stride]
 * (positive strides); Y [N, D] row-major.  With
 *   A = (1/S) sum_s |x_s - y|,   B = sum_{s<t} |x_s - x_t|   (Euclidean norms):
 *   out [N, 2]: A - B / S^2, the ensemble energy score, and A - B / (S (S - 1)), the fair one.  D = 1: the two CRPS of iwvi_sample_scores.
 * A distance is sum_d (x_sd - x_td)^2 in float32 FROM THE DIFFERENCES, then one square root -- not |x_s|^2 + |x_t|^2 - 2 x_s . x_t, which
 * loses every digit of the near pairs when the samples are tight against their offset.  The sums over pairs and samples are float64, in a
 * fixed order (lane, wave, workgroup; no atomics: two calls give the same bits); each result is rounded to float32 once.  Only the pairs
 * s < t are visited, one workgroup per point, the samples staged through LDS in tiles.
 * 2 <= S <= 16384, 1 <= D <= IWVI_MAX_P.  A point with a NaN coordinate or a NaN target gets NaN in both outputs; other points are not
 * affected.  N = 0: IWVI_OK without a launch.  IWVI_ERR_ARG before any HIP call for S, D or N (0 .. 2^31 - 1) out of range, a null
 * pointer, a non-positive stride. */
int iwvi_energy_score(const float* samples, int64_t sample_stride, int64_t point_stride, int64_t dim_stride, const float* Y,
                      int64_t N, int S, int D, float* out, void* stream);

/* Log density of each point's Gaussian kernel-density estimate on a GRID of levels, one launch (additive extension of ABI 19;
 * csrc/kde_grid.hip): the reference's conditional density picture (experiments/demo.py), 200 inputs x 10 000 samples x 200 levels.
 *   out_logdens[n, g] = logsumexp_s(-((l_ng - x_ns) / h_n)^2 / 2) - log(S h_n) - log sqrt(2 pi)
 * samples: element (s, n) at samples[s*sample_stride + n*point_stride] (positive strides, as iwvi_sample_stats; a point's samples
 *   contiguous is the fast case).  The samples are streamed through LDS, not sorted: S has no cap but S <= 2^31 - 1 - 2048.
 * levels: [G] shared by all points when level_point_stride == 0; otherwise point n's G levels start at levels + n*level_point_stride
 *   (level_point_stride >= G).  G >= 1.
 * bandwidth <= 0: Silverman's rule per point, h_n = 1.06 std_n S^(-1/5) with the population standard deviation (needs S >= 2), the
 *   formula of iwvi_kde_loglik and iwvi_sample_stats.  bandwidth > 0: that value for every point (S >= 1).  It must be finite.
 * Differences, standard deviation, bandwidth, exponents and the sum of exponentials are float64 formed from the float32 values; the sum
 * is taken relative to the exponent of the sample nearest to the level, so a level hundreds of standard deviations away gets the finite
 * value of the formula (-1e5 .. -1e6), never -inf.  The result is rounded to float32 once.  Two calls on the same inputs give the same bits.
 *   out_logdens [N, G] row-major;  out_mean_std [N, 2] or NULL: sample mean and population standard deviation;
 *   out_bandwidth [N] or NULL: the h_n actually used.
 * Silverman with all samples of a point equal: a point mass, +inf at a level equal to that value and -inf elsewhere, bandwidth 0.  A NaN
 * sample: NaN in that point's whole row, its mean, standard deviation and bandwidth; other points are not affected.  A NaN level: NaN in
 * that entry.  N == 0 returns IWVI_OK without a launch; N x ceil(G / 64) <= 2^31 - 1. */
int iwvi_kde_density_grid(const float* samples, int64_t sample_stride, int64_t point_stride, int64_t N, int64_t S,
                          const float* levels, int64_t level_point_stride, int G, double bandwidth,
                          float* out_logdens, float* out_mean_std, float* out_bandwidth, void* stream);

/* Lloyd's k-means with the semantics of scipy.cluster.vq.kmeans2's loop (additive extension of ABI 19; csrc/kmeans.hip): the first-layer
 * inducing inputs of the reference's models (experiments/build_models.py:179-180, kmeans2(X, M, minit="points")).  `iters` times:
 *   label_n = argmin_m sum_d (X[n, d] - C[m, d])^2    (dimension order; ties to the lowest m: the comparison is a strict <)
 *   C[m]    = mean of { X[n] : label_n == m }         (a centroid without members keeps its row)
 * X [N, D] and Z_init [M, D] row-major float32; everything formed from them is float64 (differences, squares, sums, means), and the
 * running centroids C stay float64 in the workspace between iterations.  The distance is the sum above as written, never the expansion
 * |x|^2 - 2 x.c + |c|^2.  1 + 2 iters launches on `stream`, nothing returns to the host in between.
 *   out_Z [M, D] float32, required: the float32 rounding of out_Z64 and nothing else; it may be Z_init.
 *   out_Z64 [M, D] or NULL: the centroids after the last update.
 *   out_labels [N] or NULL: the labels of the LAST assignment -- against the centroids before the last update, as SciPy returns them.
 *   out_counts [M] or NULL: the members at that assignment;  out_inertia [1] or NULL: the sum of the labelled points' smallest squared
 *   distances at that assignment.
 * A point with a non-finite coordinate gets label -1 and enters no sum, no count and no inertia (SciPy refuses such data; check it
 * before the call where that is wanted).  No floating-point atomics: every sum is taken in an order fixed by (N, M, D), so two calls on
 * the same inputs give the same bits.  M > N is allowed: the surplus centroids stay where Z_init put them.
 * ws: iwvi_kmeans_ws_bytes(N, M, D) bytes of device memory, contents arbitrary; at most 512 partial [M, D] sums, whatever N is.  That
 * function returns 0 for sizes iwvi_kmeans refuses.
 * IWVI_ERR_ARG (iwvi_last_error names the entry point) before any HIP call for: a null X, Z_init, out_Z or ws; N outside 1 .. 2^31 - 1;
 * D outside 1 .. IWVI_MAX_D; M outside 1 .. IWVI_MAX_M; iters < 1. */
size_t iwvi_kmeans_ws_bytes(int64_t N, int M, int D);
int iwvi_kmeans(const float* X, int64_t N, int D, const float* Z_init, int M, int iters,
                float* out_Z, double* out_Z64, int32_t* out_labels, int32_t* out_counts, double* out_inertia,
                void* ws, void* stream);

/* ------------------------------------------------------------------------
 * Likelihoods other than the Gaussian (additive extension of ABI 19; csrc/likelihood_tail.hip).  The reference hands ANY GPflow-1.x
 * likelihood object to its models and calls variational_expectations (models.py:66,134) and predict_mean_and_var (:105) on it.  The
 * non-conjugate ones integrate by Gauss-Hermite quadrature, GPflow's ndiagquad with its default 20 points:
 *   f_i = mu + sqrt(2 v) x_i,  E[g] = sum_i w_i g(f_i)   (x_i, w_i sqrt(pi)) = hermgauss(20);  the rule defines the result.
 * type         logp(F, Y)
 *   GAUSSIAN   log N(Y; F, param[0])                                     param[0] = variance   (through the same rule, which is exact for a
 *              quadratic up to rounding: a cross-check of these kernels against the fused Gaussian tail -- the models never take it)
 *   BERNOULLI  log p if Y == 1 else log(1 - p),  p = Phi(F) (1 - 2e-3) + 1e-3   (probit link with GPflow's jitter)   no parameter
 *   STUDENT_T  lgc - log s - 1/2 log(nu pi) - (nu + 1)/2 log1p(((Y - F)/s)^2 / nu)    param[0] = s (scale), param[1] = nu (df),
 *              lgc = lgamma((nu + 1)/2) - lgamma(nu/2), computed by the HOST (it depends on nu alone, and nu is not trained)
 * param0_dev: optional device scalar read instead of param[0] when the launch runs (a trained variance / scale), as lik_variance_dev.
 *
 *   MULTICLASS GPflow's MultiClass(C) with the RobustMax(C, epsilon) link (csrc/likelihood_multiclass.hip).  param[0] = epsilon in (0, 1),
 *              param[1] = C, integral, 2 <= C <= IWVI_MAX_P; lgc and param0_dev are unused; nothing is trained.  It is the one type whose
 *              targets are NOT as wide as the moments: Y is ONE column of class labels 0 .. C-1 stored as floats ([B, 1]; [rows, 1] for
 *              the elementwise entries), the moments have one column per class, and every entry must be given Dy = C.
 *                logp(F, Y) = log(1 - epsilon) if argmax_c F_c == Y (ties: the first maximum) else log(epsilon / (C - 1)).
 *              Its expectation couples the C outputs of a sample, by the same 20-point rule over the label's own output:
 *                X_i = mu_y + x_i sqrt(max(2 v_y, 1e-10)),  p = sum_i w_i prod_{c != y} [Phi((X_i - mu_c) / sqrt(max(v_c, 1e-10))) (1 - 2e-4) + 1e-4]
 *              (clips and jitter are GPflow's and part of the definition), and
 *                variational expectation = p log(1 - epsilon) + (1 - p) log(epsilon / (C - 1))               ONE value per (point, sample);
 *                predict_density         = log(p (1 - epsilon) + (1 - p) epsilon / (C - 1));
 *                predict_mean_and_var    = (P, P - P^2) [T, C],  P_k = that mixture with p evaluated for label k.
 *              iwvi_lik_var_exp and iwvi_lik_predict_density therefore write out [T, 1], iwvi_lik_predict_mean_and_var takes n = T C (a
 *              multiple of C) and writes [T, C] twice; iwvi_lik_elbo_backward writes d_mean, d_var [T, C] -- the gradient of the value
 *              as computed: zero through an active clip -- and out_sums[1] = 0.  A label outside 0 .. C-1 is read as the nearest class.
 *
 *   POISSON, EXPONENTIAL, GAMMA   GPflow's Poisson(binsize), Exponential() and Gamma(shape) with their default exp link, lambda = exp(F)
 *              (csrc/likelihood_explink.hip).  With that link the variational expectation is a CLOSED FORM, GPflow's own branch -- no
 *              quadrature, one exp per element, no variance floor (nothing divides by sqrt(v)):
 *                              logp(F, Y)                                          variational_expectations(mu, v, Y)
 *                POISSON       Y log(b l) - b l - lgamma(Y + 1)                    Y mu - b exp(mu + v/2) - lgamma(Y + 1) + Y log b
 *                EXPONENTIAL   -Y / l - log l                                      -Y exp(-mu + v/2) - mu
 *                GAMMA         -a log l - lgamma(a) + (a - 1) log Y - Y / l        -a mu - lgamma(a) + (a - 1) log Y - Y exp(-mu + v/2)
 *                conditional mean, variance:  POISSON b l, b l;  EXPONENTIAL l, l^2;  GAMMA a l, a l^2.
 *              POISSON: param[0] = b = binsize > 0, a fixed host value (param0_dev is ignored).  EXPONENTIAL: no parameter.  GAMMA:
 *              param[0] = a = shape > 0, param0_dev honoured (the one trained scalar); lgamma(a) and digamma(a) are evaluated on the
 *              device, in float64, from the value the launch reads.  lgc is unused.  Heads (exact derivatives of the closed forms), with
 *              e+ = exp(mu + v/2), e- = exp(-mu + v/2):
 *                POISSON      dE/dmu = Y - b e+,   dE/dv = -b e+ / 2
 *                EXPONENTIAL  dE/dmu = Y e- - 1,   dE/dv = -Y e- / 2
 *                GAMMA        dE/dmu = Y e- - a,   dE/dv = -Y e- / 2,   dE/da = -mu - digamma(a) + log Y   (out_sums[1]; 0 for the other two)
 *              iwvi_lik_predict_density and iwvi_lik_predict_mean_and_var are GPflow's base-class defaults by the 20-point rule above:
 *                predict_density      = log sum_i exp(logp(f_i, Y) + log w_i)                          (Fvar == NULL: logp(Fmu, Y))
 *                predict_mean_and_var = (E_y, E_y2 - E_y^2),  E_y = sum_i w_i mean(f_i),  E_y2 = sum_i w_i (var(f_i) + mean(f_i)^2);
 *              the rule defines these, not exp(mu + v/2).  The terms of the targets alone (lgamma(Y + 1), Y log b, (a - 1) log Y - lgamma(a))
 *              enter out_lse_ms[:, 0], so out_lse_ms[:, 0] + log out_lse_ms[:, 1] - log K is still the point's log p.  Targets: POISSON
 *              integers >= 0, EXPONENTIAL >= 0, GAMMA > 0 (the caller's to check).  No clamp: where exp overflows float32 (|mu +- v/2| above
 *              about 88) the formulas give +-inf or NaN, as GPflow's do in float64 at 709.
 *
 *   BETA, ORDINAL   GPflow's Beta(scale) and Ordinal(bin_edges), both through the probit link with GPflow's jitter,
 *              ip(x) = Phi(x) (1 - 2e-3) + 1e-3 (csrc/likelihood_bounded.hip).  Their values are 8 and 9: 7 is UNASSIGNED and refused as an
 *              unknown type.  Neither has a closed form: variational expectation, predict_density (in log space; Fvar == NULL: logp) and
 *              predict_mean_and_var are GPflow's base-class defaults by the 20-point rule above, as written out for the exp-link types,
 *              and the heads are its reparameterised first-derivative form (iwvi_lik_elbo_backward below), v floored at 1e-8.
 *                BETA      m = ip(F), alpha = m s, beta = s - alpha, Yc = clip(Y, 1e-6, 1 - 1e-6):
 *                          logp = (alpha - 1) log Yc + (beta - 1) log(1 - Yc) + lgamma(s) - lgamma(alpha) - lgamma(beta);
 *                          conditional mean m, variance (m - m^2) / (s + 1).
 *                          param[0] = s = scale > 0, param0_dev honoured (the one trained scalar); lgamma(s) and digamma(s) are evaluated
 *                          on the device, in float64, from the value the launch reads; digamma(alpha), digamma(beta) per node in float32.
 *                          out_sums[1] = d ELBO / d scale.  Targets in [0, 1] (the caller's to check).  param[1] and lgc are unused.
 *                ORDINAL   n strictly increasing edges e_0 .. e_(n-1) make n + 1 bins; Y holds the bin 0 .. n (as a float).  With
 *                          l = e_Y / sigma (+inf for the top bin) and r = e_(Y-1) / sigma (-inf for the bottom bin):
 *                          P_Y(F) = ip(l - F / sigma) - ip(r - F / sigma),  logp = log(P_Y + 1e-6);  the bins sum to 0.998.
 *                          conditional mean sum_j j P_j, variance sum_j j^2 P_j - mean^2.
 *                          param[1] = n, integral, 1 <= n <= IWVI_MAX_P - 1.  param0_dev is REQUIRED: 1 + n device floats
 *                          [sigma, e_0 .. e_(n-1)]; sigma (> 0, the one trained scalar) is read there by every launch and the edges behind
 *                          it.  param[0] is the host's copy of sigma and serves only to refuse sigma <= 0 before a launch.  lgc is unused.
 *                          out_sums[1] = d ELBO / d sigma.  The jitter cancels in P_Y = (1 - 2e-3)(Phi(l') - Phi(r')), and the difference is
 *                          formed on one side of 0 from erfc (across 0: from erf), never from two values near 1: float32 relative
 *                          accuracy at any distance from the bin.  A label outside 0 .. n is read as the nearest bin.
 *              IWVI_ERR_ARG (with iwvi_last_error) before any launch: BETA with param[0] <= 0 or NaN; ORDINAL with param[1] not an integer
 *              in 1..31, with param0_dev == NULL, or with param[0] <= 0 or NaN.
 *
 *   HETERO_GAUSSIAN   a Gaussian whose noise variance is a second latent function of the input (GPflow 2's heteroskedastic likelihood with the
 *              exp link; csrc/likelihood_hetero.hip).  Its value is 11: 7 and 10 are UNASSIGNED and refused as unknown types.  For Dt target
 *              columns the moments have Dy = 2 Dt columns per row: columns 0 .. Dt-1 are the mean function f, columns Dt .. 2 Dt-1 are g, the
 *              LOG NOISE VARIANCE of the same target column.  Like MULTICLASS its targets are narrower than its moments: wherever an entry
 *              point takes Dy, Y has Dy / 2 columns ([B, Dy/2]; [rows, Dy/2] for the elementwise entries), and every entry refuses a Dy that
 *              is odd, below 2 or above IWVI_MAX_P.  No parameter: param[], lgc and param0_dev are ignored (one exception, below), nothing is
 *              trained, out_sums[1] = 0.  Per target column, with (m_f, v_f) and (m_g, v_g) the moments of its two outputs:
 *                logp(F, Y)              = -1/2 log 2pi - g/2 - (y - f)^2 exp(-g) / 2
 *                variational expectation = -1/2 log 2pi - m_g/2 - ((y - m_f)^2 + v_f) r / 2,   r = exp(a),  a = -m_g + v_g/2     (closed form)
 *                heads, q = (y - m_f)^2 + v_f:  dE/dm_f = (y - m_f) r,  dE/dv_f = -r/2,  dE/dm_g = -1/2 + q r / 2,  dE/dv_g = -q r / 4
 *                predict_mean_and_var    = (m_f, v_f + exp(m_g + v_g/2))                                      (the exact moments)
 *                predict_density         = log int N(y; m_f, v_f + exp(g)) N(g; m_g, v_g) dg by the 20-point rule above over g, in log
 *                                          space: log sum_i exp(log N(y; m_f, v_f + exp(g_i)) + log w_i), g_i = m_g + sqrt(2 max(v_g, 1e-8)) x_i
 *                                          (Fvar == NULL: logp(Fmu, Y))
 *                mixture over S draws    mean: the average of m_f; variance: the average of v_f + exp(m_g + v_g/2) + m_f^2 minus the mean
 *                                          squared; log density: logsumexp_s sum_d predict_density_s - log S
 *                sample_y                f = m_f + sqrt(v_f) z_1,  g = m_g + sqrt(v_g) z_2,  y = f + exp(g/2) eps
 *              THE CLIP: every exponent (a, -g, m_g + v_g/2, the nodes g_i, g/2) is clipped to [-60, 60] before exp, so float32 cannot
 *              overflow.  The heads are the gradient of the value AS COMPUTED: through an active clip (|a| > 60) the derivative is zero --
 *              the m_g / v_g parts through r vanish (dE/dm_g = -1/2, dE/dv_g = 0) while dE/dm_f and dE/dv_f keep the clipped r --, as for
 *              MULTICLASS.  The outputs of iwvi_lik_var_exp, iwvi_lik_predict_density, iwvi_lik_predict_mean_and_var and the out_mean /
 *              out_var of iwvi_lik_predict_mixture are [., Dy/2]; d_mean, d_var of iwvi_lik_elbo_backward, z_f and out_f of
 *              iwvi_lik_sample_y are [., Dy] (z_f supplies z_1 in column d and z_2 in column Dy/2 + d); out_y of iwvi_lik_sample_y is
 *              [T, Dy/2].  Targets: any finite real.
 *              The exception: iwvi_lik_predict_mean_and_var has no Dy argument, so for this type it reads the row width Dy from param[1]
 *              (as MULTICLASS's C), takes n = T Dy elements of moments and writes [T, Dy/2] twice.
 * ---------------------------------------------------------------------- */
enum { IWVI_LIK_GAUSSIAN = 0, IWVI_LIK_BERNOULLI_PROBIT = 1, IWVI_LIK_STUDENT_T = 2, IWVI_LIK_MULTICLASS = 3,
       IWVI_LIK_POISSON = 4, IWVI_LIK_EXPONENTIAL = 5, IWVI_LIK_GAMMA = 6, /* 7: unassigned, refused as unknown */
       IWVI_LIK_BETA = 8, IWVI_LIK_ORDINAL = 9, /* 10: unassigned, refused as unknown */
       IWVI_LIK_HETERO_GAUSSIAN = 11 };
typedef struct iwvi_lik_desc {
    int32_t type;
    float param[2];
    float lgc;
    const float* param0_dev;
} iwvi_lik_desc;

/* iwvi_iw_elbo_reduce_dev with a likelihood descriptor in place of lik_variance: the variational expectation of every (point, sample,
 * output) by the rule above, everything else -- strides, regularisers, ticket, optional outputs, ONE launch -- as documented there.
 * HETERO_GAUSSIAN: Dy = 2 Dt is the width of the moments, Y is [B, Dy / 2]; the expectation is its closed form, summed over the Dt columns. */
int iwvi_lik_elbo_reduce(const iwvi_lik_desc* lik, const float* fmean, const float* fvar, const float* Y,
                         int64_t B, int K, int Dy, int64_t stride_b, int64_t stride_k,
                         const float* const* kl_local_host, const int32_t* kl_dims_host, int n_kl,
                         const double* const* kl_global_host, const int32_t* kl_global_counts_host, int n_glob,
                         double scale, int K_total, int mode_vi,
                         float* out_lse_ms, float* out_logp, double* out_elbo, uint64_t* ticket, void* stream);

/* iwvi_iw_elbo_backward_dev with a likelihood descriptor: out_w, d_mean, d_var, out_sums[0] and [2] as there, out_sums[1] =
 * d ELBO / d param[0] (0 for the Bernoulli; BETA: d / d scale; ORDINAL: d / d sigma, the head of param0_dev).  The heads use the reparameterised form of the rule, first derivatives only:
 *   dE/dmu = sum_i w_i g'(f_i),   dE/dv = sum_i w_i g'(f_i) x_i / sqrt(2 v)   with v floored at 1e-8.
 * HETERO_GAUSSIAN: Y is [B, Dy / 2], d_mean and d_var are [B K, Dy] (the closed-form heads of the table above, zero through an active clip),
 * out_sums[1] = 0. */
int iwvi_lik_elbo_backward(const iwvi_lik_desc* lik, const float* fmean, const float* fvar, const float* Y, int Dy,
                           const float* const* kl_local, const int32_t* kl_dims, int n_local,
                           int64_t B, int K, double scale, int mode_vi,
                           float* out_w, float* d_mean, float* d_var,
                           const double* const* kl_global, const int32_t* kl_global_counts, int n_glob,
                           const float* lse_global, int K_total,
                           double* out_sums, double* ws, void* stream);

/* The likelihood's methods as elementwise callables on explicit moments, Fmu / Fvar / out [T, Dy], Y row (t / row_div) % row_mod as in
 * iwvi_gaussian_var_exp.  iwvi_lik_predict_density: log of the predictive density (the Bernoulli's closed form at
 * p = inv_probit(Fmu / sqrt(1 + Fvar)), the Student-t's log-space quadrature of logp); Fvar == NULL: logp(Fmu, Y).
 * iwvi_lik_predict_mean_and_var (n elements): Bernoulli (p, p - p^2) at that p; Student-t (Fmu, E[s^2 nu/(nu - 2) + F^2] - Fmu^2) by the
 * rule, nu > 2 required; Gaussian (Fmu, Fvar + variance); the exp-link types, BETA and ORDINAL: the rule over the conditional moments.
 * HETERO_GAUSSIAN: Fmu / Fvar are [T, Dy], Y's rows and out are [., Dy / 2] (one value per row and target column);
 * iwvi_lik_predict_mean_and_var takes n = T Dy with Dy in param[1] and writes out_mean, out_var [T, Dy / 2]. */
int iwvi_lik_var_exp(const iwvi_lik_desc* lik, const float* Fmu, const float* Fvar, const float* Y,
                     int64_t T, int Dy, int64_t row_div, int64_t row_mod, float* out, void* stream);
int iwvi_lik_predict_density(const iwvi_lik_desc* lik, const float* Fmu, const float* Fvar, const float* Y,
                             int64_t T, int Dy, int64_t row_div, int64_t row_mod, float* out, void* stream);
int iwvi_lik_predict_mean_and_var(const iwvi_lik_desc* lik, const float* Fmu, const float* Fvar, int64_t n,
                                  float* out_mean, float* out_var, void* stream);

/* The Monte Carlo predictive MIXTURE of a test point over S draws through the inner layers, on the final layer's moments of those draws
 * (additive extension of ABI 19).  Per test point n, over its S draws s (moments row n*stride_n + s*stride_s, Dy columns):
 *   out_logp[n]    = logsumexp_s( sum_d predict_density(fmean, fvar, Y[n, d]) ) - log S        (Y, out_logp: both or neither)
 *   out_mean[n, d] = (1/S) sum_s E_s[y_d]
 *   out_var [n, d] = (1/S) sum_s (Var_s[y_d] + E_s[y_d]^2) - out_mean[n, d]^2                  (law of total variance)
 * predict_density and (E_s, Var_s) = predict_mean_and_var are exactly what the elementwise entries above compute for the type (the same
 * device functions).  MULTICLASS: Dy = C, Y is [N, 1] of labels, out_mean = the class probabilities averaged over the draws, out_var =
 * P - P^2 of those; the C probabilities of a draw are evaluated once and the label's density is the logarithm of its own.
 * Layouts: point-major rows n S + s (stride_n = S, stride_s = 1) or sample-major rows s N + n (stride_n = 1, stride_s = N); strides >= 0.
 * ONE launch, no workspace, no ticket, no host synchronisation: capturable in a hipGraph.  Arithmetic: float32 inside a draw; the
 * log-sum-exp is shifted by the running float32 maximum and summed in float64 (a point whose every draw has density -inf gives -inf, not
 * NaN); sum_s E_s and sum_s (Var_s + E_s^2) accumulate in float64 and out_var is formed there and rounded once.  The exp-link types add a
 * point's target-only terms (sum_d c0(y_d)) once, outside the log-sum-exp.
 * HETERO_GAUSSIAN: Dy = 2 Dt, Y is [N, Dy / 2], out_mean and out_var are [N, Dy / 2]; a draw's density is the sum over its Dt target columns.
 * Any output may be NULL, at least one must be given, out_mean and out_var go together.  Every type is accepted -- the Gaussian's
 * out_logp is what iwvi_dgp_predict_density computes from the same moments: a cross-check.  A Student-t with df <= 2 is refused only when
 * the moments are asked for.  IWVI_ERR_ARG (with iwvi_last_error) before any launch for: a null or invalid descriptor, N < 0, S < 1, Dy
 * outside 1..IWVI_MAX_P, MULTICLASS with Dy != C, HETERO_GAUSSIAN with an odd Dy, out_logp without Y or Y without out_logp, out_mean without out_var or the reverse, no
 * output at all.  N = 0: IWVI_OK, nothing is launched. */
int iwvi_lik_predict_mixture(const iwvi_lik_desc* lik, const float* fmean, const float* fvar, const float* Y,
                             int64_t N, int S, int Dy, int64_t stride_n, int64_t stride_s,
                             float* out_logp, float* out_mean, float* out_var, void* stream);

/* Importance-weight summaries of S draws per point in one launch (additive extension of ABI 19; csrc/psis.hip): the importance-sampled
 * log density log (1/S) sum_s w_s, Kish's effective sample size, and Pareto-smoothed importance sampling with its diagnostic khat
 * (Vehtari, Simpson, Gelman, Yao, Gabry, "Pareto smoothed importance sampling"; the generalized-Pareto fit of Zhang & Stephens 2009 with
 * the PSIS prior).  khat < 0.5: good; 0.5 <= khat < 0.7: usable; khat >= 0.7: the estimate is not reliable at any practical S.
 * Per point n over its S draws s, every per-row array read at row n*stride_n + s*stride_s (strides >= 0), the log-weight l_ns is
 *   terms mode    (terms [rows, n_terms], 1 <= n_terms <= IWVI_MAX_P):   l = sum_j terms[row, j] - sum_i sum_c kl_local[i][row, c]
 *                 n_terms = 1, n_kl = 0 summarises given log-weights [N, S] in any strides -- the training log-weights included; the
 *                 columns of iwvi_lik_predict_density / iwvi_lik_var_exp are the terms of every likelihood but the Gaussian
 *   moments mode  (terms == NULL; fmean, fvar [rows, Dy], Y [N, Dy], the Gaussian's variance lik_variance or, if given, *lik_variance_dev):
 *                 var_exp = 0:  l = sum_d log N(y; m, v + s) - sum kl         (the predictive density of the draw)
 *                 var_exp = 1:  l = sum_d [log N(y; m, s) - v / (2 s)] - sum kl   (the bound's own term)
 * kl_local: n_kl <= IWVI_MAX_KL device arrays [rows, kl_dims[i]] (a host array of pointers, read during the call): each latent-variable
 * layer's sampled log q(w) - log p(w).  Outputs, each [N] but out_logw [N, S] (point-major), any may be NULL, at least one is required:
 *   out_logw  l_ns                                    out_raw   logsumexp_s l - log S
 *   out_ess   (sum_s w)^2 / sum_s w^2, in [1, S], as iwvi_bound_logw_reduce
 *   out_khat, out_psis:  x = sort(l - max l); M = ceil(min(S / 5, 3 sqrt S)); cutoff = max(x[S - M - 1], log 2^-126); the tail is the
 *             n entries STRICTLY above the cutoff.  n <= 4 (S < 21, all weights equal, ..): khat = +inf and psis = raw.  Otherwise, on the
 *             exceedances e = exp(tail) - exp(cutoff), ascending:  m = 30 + floor(sqrt n);  b_j = (1 - sqrt(m / (j - 1/2))) / (3 e[floor(n/4
 *             + 1/2) - 1]) + 1 / e[n - 1];  k_j = mean log1p(-b_j e);  L_j = n (log(-b_j / k_j) - k_j - 1);  w = softmax(L), entries below
 *             10 * 2^-52 dropped and the rest renormalised;  b = sum w_j b_j;  k = mean log1p(-b e);  sigma = -k / b;
 *             khat = (n k + 5) / (n + 10).  The tail's i-th log-weight (i = 1 .. n) becomes min(log(sigma expm1(-khat log1p(-p_i)) / khat
 *             + exp(cutoff)), 0), p_i = (i - 1/2) / n (-sigma log1p(-p_i) when |khat| < 2^-52), and out_psis is the log-mean of the
 *             weights with that tail.  khat or sigma not finite: the tail stays as it is (psis = raw).
 * A -inf log-weight is a zero weight; every draw at -inf: raw = psis = -inf, ess = 0, khat = +inf.  A NaN log-weight -- or a +inf one,
 * which leaves the others no weight to be relative to -- gives NaN in the point's four summaries; other points are not affected.
 * Arithmetic: float32 inside a draw; exp(l - max l) in float32, every sum in float64; everything from the exceedances on in float64; each
 * result rounded to float32 once.  ONE launch, no workspace, no atomics, no ticket, no host synchronisation: two calls give the same bits,
 * and the launch is capturable in a hipGraph.  One sort per point in LDS (csrc/sample_sort.h), four, two or one point per workgroup by S.
 * IWVI_ERR_ARG (with iwvi_last_error) before any launch for: a null descriptor, N outside 0 .. 2^31 - 1, S outside 1 .. 16384, a negative
 * stride, neither terms nor moments or both, n_terms or Dy outside 1..IWVI_MAX_P, n_kl outside 0..IWVI_MAX_KL, a NULL kl_local pointer,
 * a kl_dims entry below 1, moments without Y, lik_variance <= 0 or NaN, no output at all.  N = 0: IWVI_OK, nothing is launched. */
typedef struct iwvi_psis_desc {
    const float* terms;
    int32_t n_terms;
    const float* fmean;
    const float* fvar;
    const float* Y;
    int32_t Dy;
    int32_t var_exp;
    float lik_variance;
    const float* lik_variance_dev;
    const float* const* kl_local;
    const int32_t* kl_dims;
    int32_t n_kl;
    int64_t N;
    int32_t S;
    int64_t stride_n;
    int64_t stride_s;
    float* out_logw;
    float* out_raw;
    float* out_ess;
    float* out_khat;
    float* out_psis;
} iwvi_psis_desc;
int iwvi_psis_summary(const iwvi_psis_desc* desc, void* stream);

/* Exact draws of a predictive target, y ~ p(y | f) with f ~ N(fmean, fvar), for every likelihood above (additive extension of ABI 19;
 * csrc/likelihood_sample.hip).  fmean, fvar [T, Dy]: the final layer's moments, one row per (point, draw) in either layout -- the kernel is
 * elementwise over rows.  fvar == NULL: f = fmean.  z_f: optional [T, Dy] standard normals for f (tests); otherwise they are drawn.
 * out_f: optional [T, Dy], the f that was used (the exported noise: a test conditions on it).  out_y [T, Dt], Dt = Dy, except MULTICLASS:
 * Dy = C and Dt = 1 (one label column), and HETERO_GAUSSIAN: Dt = Dy / 2 (z_f and out_f stay [T, Dy]).  f = fmean + sqrt(max(fvar, 0)) z; links and jitters as in the table above:
 *   GAUSSIAN     y = f + sqrt(variance) e
 *   BERNOULLI    y = 1 with probability ip(f) = Phi(f) (1 - 2e-3) + 1e-3, else 0
 *   STUDENT_T    y = f + s n / sqrt(g / (nu / 2)),  n ~ N(0, 1), g ~ Gamma(nu / 2, 1); any nu > 0
 *   MULTICLASS   the first arg-max of f_1 .. f_C with probability 1 - epsilon, otherwise one of the other C - 1 classes, uniformly
 *   POISSON      y ~ Poisson(b exp(f)), exact: sequential inversion below a rate of 10, Hoermann's transformed rejection (PTRS) from 10 on,
 *                round(rate + sqrt(rate) n) from 2^24 on (float32 no longer holds the integers); a rate of +inf gives +inf
 *   EXPONENTIAL  y = -exp(f) log u, u in (0, 1]
 *   GAMMA        y = exp(f) G, G ~ Gamma(a, 1) by Marsaglia-Tsang; a < 1: Gamma(a + 1) u^(1/a), formed in log space
 *   BETA         alpha = ip(f) s, beta = s - alpha, y = G_alpha / (G_alpha + G_beta)
 *   ORDINAL      bin j with probability P_j(f) / sum_k P_k(f) (the P_j sum to 0.998): inverse CDF over the n + 1 bins from one uniform
 *   HETERO_GAUSSIAN  per target column d: f = column d, g = column Dy/2 + d of that formula, y = f + exp(clip(g / 2)) e; the element (and
 *                sub-stream) is t Dy/2 + d; round 0 gives z_1 and e (words 0, 1) and z_2 (words 2, 3)
 * A NaN moment gives a NaN y.  param0_dev is honoured as everywhere: trained variance, scale, shape and sigma are read on the device.
 * EVERY LOOP IS CAPPED: a rejection sampler (Marsaglia-Tsang, PTRS) runs at most 32 rounds -- exhaustion probability below 0.14^32 = 5e-28
 * at their acceptance rates -- and then returns the conditional mean (f; a exp(f); ip(f); the rate, rounded); the Poisson inversion takes at
 * most 64 steps (P(Poisson(10) > 64) < 1e-29); the Ordinal walks its n edges, the MultiClass its C classes.
 * Randomness: Philox4x32-10, one sub-stream per ELEMENT (draw consumption varies): counter = (element index low, high, round, serial low),
 * key = (seed low, seed high ^ serial high); element = t Dy + d.  Round 0 gives z, a second normal and two uniforms; rounds 1 .. 32 (BETA:
 * 33 .. 64 for G_beta) feed one rejection round each.  The same (seed, serial) gives the same bits.  serial_dev, if given, is ONE device
 * word read instead of `serial`: its low 32 bits are the serial, its high 32 bits count the arrivals of the running launch (zero the word
 * once).  Every workgroup reads the serial, the last one to finish clears the count and adds one to the serial (the ticket of
 * iwvi_fill_normal_dev, kept in the word itself): replays of a captured graph draw fresh values; launches sharing a word must be
 * stream-ordered.  The device serial is 32 bits wide: the key's hi32(serial) term is 0 with serial_dev, and the word must be re-zeroed
 * before its 2^32nd launch (the increment would carry into the arrival count).
 * ONE launch, no workspace, no host synchronisation: capturable in a hipGraph.  T = 0: IWVI_OK, nothing is launched.  IWVI_ERR_ARG (with
 * iwvi_last_error) before any launch: a null or invalid descriptor (the checks of iwvi_lik_predict_mixture), T < 0, Dy outside
 * 1..IWVI_MAX_P, MULTICLASS with Dy != C, HETERO_GAUSSIAN with an odd Dy, a null out_y (or, with T > 0, a null fmean). */
int iwvi_lik_sample_y(const iwvi_lik_desc* lik, const float* fmean, const float* fvar, int64_t T, int Dy, const float* z_f,
                      uint64_t seed, uint64_t serial, uint64_t* serial_dev, float* out_y, float* out_f, void* stream);

/* white=False (temp_workaround.py:63-65: "another backsubstitution in the unwhitened case").  The unwhitened
 * q(u) = N(f, q_sqrt q_sqrt^T) gives the same conditional as the whitened one with f_w = Lm^-1 f and
 * q_sqrt_w[r] = Lm^-1 tril(q_sqrt[r]) (lower triangular again), so the back-substitution is applied ONCE to the
 * operands (float64 accumulate) instead of per sample; the caller then runs iwvi_gp_precompute on (f_w, q_sqrt_w).
 * state: precomputed WITH IWVI_GP_WANT_DENSE for the same (M, R) (the dense Lm^-1 is read);
 * f [M, R], q_sqrt [R, M, M] or NULL -> f_w [M, R], q_sqrt_w [R, M, M]. */
int iwvi_unwhiten(const void* state, int M, int R, const float* f, const float* q_sqrt,
                  float* f_w, float* q_sqrt_w, void* stream);

/* counter-based N(0,1) fill (Philox4x32-10 + Box-Muller); stream documented in DESIGN.md */
int iwvi_fill_normal(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
/* same stream, but the counter lives on the device: state[0] = counter (read by every block of the launch, then advanced by
 * ceil(n/4) by the last block to finish), state[1] = the launch's arrival ticket (every block adds to it once, the last one
 * leaves it at 0); zero both once.  Launches of any sizes may share one state as long as they cannot overlap in time (one
 * stream, or ordered by events): launch i then draws the stream from the sum of the earlier ceil(n/4).  Lets a captured
 * hipGraph draw fresh noise on every replay. */
int iwvi_fill_normal_dev(float* out, int64_t n, uint64_t seed, uint64_t* state, void* stream);

/* The SGHMC inference mode (experiments/sghmc.py; csrc/sghmc.hip).
 * iwvi_neg_log_prior: -log N(q_mu; 0, I) of a whitened q_mu [M, R] = 1/2 |q_mu|_F^2 + 1/2 M R log 2 pi -> out [1] double: the global
 * regulariser of a GP layer without q_sqrt (temp_workaround.py:167-184), in place of KL[q(u) || p(u)].
 * iwvi_sghmc_step: one launch updates every sampled tensor (at most IWVI_SGHMC_MAX_TENSORS).  Per element, every right-hand side reading the
 * values from BEFORE the step, with grad = -`grad` (`grad` holds d bound / d theta as the adjoints leave it; the sampler descends -bound):
 *   r = 1 / (xi + 1);  g' = (1 - r) g + r grad;  g2' = (1 - r) g2 + r grad^2;  xi' = 1 + xi (1 - g^2 / (g2 + 1e-16));
 *   Minv = 1 / (sqrt(g2 + 1e-16) + 1e-16);  sigma = sqrt(max(2 (epsilon / sqrt(num_data))^2 mdecay Minv, 1e-16));
 *   p' = p - epsilon^2 Minv grad - mdecay p + sigma n;  theta' = theta + p'.
 * burn_in != 0 writes xi', g', g2' as well as p' and theta' (the reference's burn_in_op), burn_in == 0 writes p' and theta' only
 * (sample_op).  Arithmetic in float64 without contraction; theta64 is the float64 master of theta (set it to theta once), `theta` receives
 * its float32 rounding.  Noise n ~ N(0, 1): `noise` [n] float32 if given, else drawn from Philox4x32-10 + Box-Muller with key `seed` and the
 * counter on the device, rng_state = {counter, arrival ticket} as for iwvi_fill_normal_dev (zero both once; launches sharing a state must
 * not overlap in time).  The tensors WITHOUT injected noise share the counter in descriptor order: with c = the counter before the launch
 * and o_i = the sum of ceil(n_j / 4) over the drawing tensors j < i, tensor i draws exactly what iwvi_fill_normal(out, n_i, seed, c + o_i)
 * writes; the launch advances the counter by the sum over all drawing tensors, so a captured hipGraph draws fresh noise on every replay.
 * `noise_out` [n] (optional) receives the n that was used.  rng_state may be NULL when every tensor has injected noise.
 * IWVI_ERR_ARG (with iwvi_last_error) before any HIP call for a null pointer, n <= 0, a tensor count outside 1 .. IWVI_SGHMC_MAX_TENSORS,
 * epsilon <= 0, mdecay < 0, num_data <= 0, a non-finite scalar, or a drawing tensor without rng_state. */
#define IWVI_SGHMC_MAX_TENSORS 8
typedef struct iwvi_sghmc_tensor {
    float* theta; const float* grad; double* xi; double* g; double* g2; double* p; double* theta64;
    const float* noise; float* noise_out; int64_t n;
} iwvi_sghmc_tensor;
int iwvi_sghmc_step(const iwvi_sghmc_tensor* tensors_host, int n_tensors, double epsilon, double mdecay, double num_data,
                    int burn_in, uint64_t seed, uint64_t* rng_state, void* stream);
int iwvi_neg_log_prior(const float* q_mu, int M, int R, double* out, void* stream);

/* ------------------------------------------------------------------------
 * The CVAE baseline (additive extension of ABI 19; csrc/cvae.hip; reference experiments/build_models.py:29-142): an MLP encoder and an MLP
 * decoder in float32, NO skip connections (unlike the Encoder of the latent-variable layer above).
 *   encoder  [x, y] -> (means | raw) [2L]   widths enc_dims = [Dx + Dy, hidden.., 2L];  hidden activation after every map but the last
 *   raw_c = clip(raw, ln 1e-12, ln 1e10) (zero gradient outside, as tf.clip_by_value);  sigma = exp(raw_c / 2);  z = mu + eps sigma
 *   decoder  [z, x] -> yhat [Dy]            widths dec_dims = [L + Dx, hidden.., Dy] (the same hidden widths), z FIRST
 *   out[0] = elbo = out[1] - out[2],  out[1] = sum_{n,d} log N(y_nd; yhat_nd, variance),  out[2] = sum_{n,j} KL(N(mu_nj, sigma_nj^2) || N(0, 1))
 * Both sums run over the B rows given; no N / B scale (the reference applies none).  W[i] is [dims[i], dims[i+1]] row-major, b[i] [dims[i+1]].
 * variance = *variance_dev when that device scalar is given.
 *
 * Launch structure.  A row-parallel launch takes eight rows per workgroup through encoder, clip, sample, decoder, the per-row log density and
 * KL and -- gradient entry only -- the deltas of every map, activations in LDS; every map's input rows and deltas go to the workspace.  The
 * second launch of the gradient entry forms dW = A^T Delta and db of every map in 8 x 8 tiles, each entry summing the rows in a fixed order,
 * and its last workgroup sums the per-workgroup (log p, KL, d variance) partials in float64 in a fixed order; the value entry's second
 * launch is that last workgroup alone.  No float atomics: two calls on the same inputs give the same bits, and the value entry's three
 * scalars are bit-identical to the gradient entry's.  iwvi_cvae_elbo_and_grad does not run the value entry.
 *
 * Noise.  eps [B, L] if given; otherwise the launch draws exactly what iwvi_fill_normal(out, B L, seed, c) writes, c = rng_state[0], and the
 * entry's second launch advances the counter by ceil(B L / 4) (the protocol of iwvi_sghmc_step; rng_state[1] is left as it is found).
 * eps_out [B, L] (optional) receives what was used.  rng_state may be NULL when eps is given.
 * ws: iwvi_cvae_ws_bytes(desc, B) bytes of device memory, 256-byte aligned, no initial contents (0 for B <= 0 or an invalid descriptor).
 *
 * iwvi_cvae_predict_samples: out_y[n, s, d] = decoder(z_t, x_n)_d + sqrt(variance) z_y[t, d], t = n S + s -- [N, S, Dy], a point's S samples
 * contiguous (what iwvi_dgp_predict_samples writes and iwvi_sample_stats reads fastest); ONE launch.  z [N S, L] and z_y [N S, Dy] may be
 * injected; a missing one is drawn: z as iwvi_fill_normal(., N S L, seed, c), z_y as iwvi_fill_normal(., N S Dy, seed, c + ceil(N S L / 4)),
 * and a launch that draws anything advances the counter by ceil(N S L / 4) + ceil(N S Dy / 4) (rng_state = {counter, arrival ticket} as for
 * iwvi_fill_normal_dev).  flags & IWVI_CVAE_NO_Y_NOISE: the decoder's output alone (predict_y), z_y is neither read nor drawn.
 * N S < 2^31 - 4096.
 *
 * IWVI_ERR_ARG (iwvi_last_error names the entry point) before any HIP call for: a null pointer, B / N / S <= 0, n_maps outside
 * 1 .. IWVI_CVAE_MAX_MAPS, a width outside 1 .. IWVI_CVAE_MAX_WIDTH, L outside 1 .. IWVI_CVAE_MAX_L, Dy outside 1 .. IWVI_CVAE_MAX_DY,
 * enc_dims[0] != Dx + Dy, dec_dims[0] != L + Dx, enc_dims[last] != 2 L, dec_dims[last] != Dy, hidden widths that differ between the two
 * nets, an unknown activation, a missing workspace, a drawing call without rng_state, N S out of range.
 * ---------------------------------------------------------------------- */
#define IWVI_CVAE_MAX_MAPS 4     /* linear maps per net ('100_100_100')                    */
#define IWVI_CVAE_MAX_WIDTH 128  /* every width, Dx + Dy and L + Dx included               */
#define IWVI_CVAE_MAX_L 8        /* latent dimensions                                      */
#define IWVI_CVAE_MAX_DY 8       /* target columns                                         */
#define IWVI_CVAE_NO_Y_NOISE 1   /* iwvi_cvae_predict_samples flags                        */
typedef struct iwvi_cvae_desc {
    const float* const* enc_W; const float* const* enc_b;   /* host arrays of n_maps device pointers */
    const float* const* dec_W; const float* const* dec_b;
    const int32_t* enc_dims; const int32_t* dec_dims;       /* host: n_maps + 1 widths each          */
    int32_t n_maps;                                         /* linear maps per net                   */
    int32_t Dx, Dy, L;
    int32_t act;                                            /* IWVI_ACT_* of the hidden layers       */
    float variance;
    const float* variance_dev;                              /* optional device scalar, wins when given */
} iwvi_cvae_desc;
typedef struct iwvi_cvae_grads {                            /* d elbo / d parameter, shaped like the parameters */
    float* const* enc_dW; float* const* enc_db;             /* host arrays of n_maps device pointers */
    float* const* dec_dW; float* const* dec_db;
    double* dvariance;                                      /* [1] float64 (feeds IWVI_ADAM_GRAD_F64) */
} iwvi_cvae_grads;
size_t iwvi_cvae_ws_bytes(const iwvi_cvae_desc* desc, int64_t B);
int iwvi_cvae_elbo(const iwvi_cvae_desc* desc, const float* X, const float* Y, int64_t B, const float* eps, uint64_t seed,
                   uint64_t* rng_state, float* eps_out, double* out, void* ws, void* stream);
int iwvi_cvae_elbo_and_grad(const iwvi_cvae_desc* desc, const float* X, const float* Y, int64_t B, const float* eps, uint64_t seed,
                            uint64_t* rng_state, float* eps_out, double* out, const iwvi_cvae_grads* grads, void* ws, void* stream);
int iwvi_cvae_predict_samples(const iwvi_cvae_desc* desc, const float* X, int64_t N, int64_t S, const float* z, const float* z_y,
                              int flags, uint64_t seed, uint64_t* rng_state, float* out_y, void* stream);

/* Diagnostic / development route switches (NOT part of the drop-in surface, like iwvi_debug_set_stamps): the library itself never reads
 * the environment.  name = one of the IWVI_* route names listed in csrc/abi.hip (e.g. "IWVI_BW_FUSED", "IWVI_NATGRAD_UNFUSED"),
 * value 0 = default route.  Returns 0, or IWVI_ERR_ARG for an unknown name.  Process-wide; not for concurrent use with launches. */
int iwvi_debug_set_option(const char* name, int value);
/* Which instantiation of the fused forward kernel the LAST iwvi_dgp_forward call of this process launched (tests assert that a shape
 * takes / does not take the compiled-in-shapes variants): bits 0-7 sub-tiles per workgroup (NS), bit 8 split-f16 stage 2, bit 9 the
 * large-M (M > 128) build, bits 10-11 LEAN mode (0 general, 1 bound-only, 2 with per-layer outputs), bit 12 a layer ran the float64
 * stage-1 route.  0 before the first launch. */
int iwvi_debug_last_forward_variant(void);
/* The plan of a fused-forward call without the call: the arguments of iwvi_dgp_forward (stream is not read) go through every check and
 * decision of the host driver, and on success out_host[0..2] receive the word iwvi_debug_last_forward_variant() would report after the
 * launch, the grid (workgroups) and the dynamic LDS bytes.  A refusal returns the status and error text of the entry it stands for.
 * No HIP function is called and no data pointer is dereferenced (only the descriptors and their encoder tables are read), so it runs on
 * a host without a device; the pointers only need to be null or not as in the real call.  tail selects the entry: the bound
 * (iwvi_dgp_forward), or one of the predictive entries with their own checks -- then N = row_mod, S = row_div, T is not read, the
 * variance is lik_variance, out_logw stands for out_logp and ws (density) or out_y (samples) and XY for z_y (samples). */
#define IWVI_FW_TAIL_BOUND 0
#define IWVI_FW_TAIL_DENSITY 1
#define IWVI_FW_TAIL_SAMPLES 2
int iwvi_debug_forward_plan(const iwvi_layer_desc* layers, int n_layers, const float* X, int Dx, const float* XY, int XYdim,
                            const float* Y, int Dy, int64_t T, int64_t row_div, int64_t row_mod, float lik_variance, uint64_t seed,
                            uint64_t* rng_state, float* out_logw, const iwvi_elbo_desc* elbo, void* stream, int tail, int64_t* out_host);
/* In-kernel time stamps of the fused forward / of the precompute launch (128 64-bit words per workgroup; NULL switches them off) and an
 * early exit of the fused forward after phase N -- timing scripts only (scripts/stamp_*.py, bench.py's gemm_phase_mfma_util). */
/* ABI 18: the route of every GP layer adjoint (iwvi_gp_layer_backward) since the previous call of this function, in call order (the latest
 * IWVI_MAX_STACK are kept): 3 ints per layer in out_host -- the route (IWVI_BW_ROUTE_*), the input-dimension bucket of the kernel-adjoint
 * template that ran (8 / 16 / 32 for the chain and the fused kernel, 4 / 8 / 16 / 32 for the GEMM route's k_bw_kernel, 0 where no kernel
 * adjoint ran) and the samples per workgroup of that kernel.  Writes at most `max` layers, returns how many were recorded, empties the log. */
#define IWVI_BW_ROUTE_CHAIN 1   /* k_bw_chain: the streaming per-sample chain             */
#define IWVI_BW_ROUTE_MID 2     /* k_bw_mid: heads + dA + dK + kernel adjoint in one launch */
#define IWVI_BW_ROUTE_GEMM 3    /* k_bw_heads, the GEMMs over u_out, k_bw_kernel          */
int iwvi_debug_last_backward_routes(int* out_host, int max);
void iwvi_debug_set_stamps(void* buf, int64_t max_workgroups);
void iwvi_debug_set_pre_stamps(void* buf);
void iwvi_debug_set_exit(int phase);

#ifdef __cplusplus
}
#endif
#endif /* IWVI_HIP_H */
