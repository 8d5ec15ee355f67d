"""Model classes of the reference's ``dgps_with_iwvi/models.py`` (DGP_VI :9-107, DGP_IWVI :110-150)
with the same constructor / method signatures, running on the HIP kernels behind include/iwvi_hip.h.

``DGP_IWVI._build_likelihood`` is the north-star function; ``E_log_p_Y`` (the name used in the older
doubly-stochastic DGP code and in BASELINE.json) is an alias for its per-point log-weight stage.

One ELBO evaluation is TWO launches: ``iwvi_model_precompute`` (per GP layer: Gram + float64 Cholesky + operand packing; the
encoders of the latent-variable layers) and ``iwvi_dgp_forward``, whose workgroups each carry a chunk of samples through the
tiling of X/Y over K, every layer, the Gaussian variational expectation and the local regularisers in LDS; the last workgroup
to finish does the log-sum-exp over K, the scaled sum and subtracts the global KLs.

A likelihood other than the Gaussian (``likelihoods.Bernoulli`` / ``StudentT`` / ``MultiClass`` / ``Poisson`` / ``Exponential`` / ``Gamma`` / ``Beta`` / ``Ordinal``) takes THREE: the layer launch runs without its tail and leaves
the final layer's moments and the local regularisers, ``iwvi_lik_elbo_reduce`` does the rest (Gauss-Hermite variational expectations -- closed
forms for the exp-link three --, the log-sum-exp, the bound).  For a Gaussian nothing differs from the two-launch form.  ``MultiClass`` alone has targets narrower than the
final layer -- Y is one column of class labels, the layer has one output per class --: ``likelihoods.target_dim`` / ``output_dim`` translate;
``HeteroskedasticGaussian`` has two outputs (mean, log noise variance) per target column and goes through the same two functions.
``predict_mixture`` evaluates a trained model of any likelihood the same way: the layer launch, then one ``iwvi_lik_predict_mixture`` launch gives
the mean, variance and log density of the Monte Carlo predictive mixture over S draws (``predict_log_density`` of a non-Gaussian model is its density).
``importance_log_density`` is the held-out log density with the encoders as the proposal instead of the prior: the layer launch with the
sampled local regularisers, then one ``iwvi_psis_summary`` launch gives the importance-sampled estimate, its Pareto-smoothed form, the
Pareto-k diagnostic and the effective sample size per point.

Differences from the reference, all documented in DESIGN.md:
  * ``zs`` (one N(0,1) array or None per layer) injects the noise tf.random_normal draws in-graph; None
    draws inside the kernel from a counter-based Philox stream (``settings.seed``, per-model step counter);
  * the IW path asks the final layer for marginal variances only (``full_cov_over_samples=False``):
    the reference builds the [B, Dy, K, K] covariance and keeps its diagonal (models.py:129-133),
    the result is identical; set the flag to follow the reference literally (layer-by-layer launches).
    Inner layers: a SharedMixedMok layer samples marginally in the reference too (temp_workaround.py:125-129), so the
    fused launch is exact for the benchmark family; an inner GPLayer with a PLAIN kernel draws its K samples per point
    jointly there (:149-155, full_cov=True) -- such a model is detected (``_joint_over_samples``) and evaluated along
    the literal layer-by-layer path, never with marginal draws.
"""
import ctypes

import numpy as np
import torch

from . import _abi, settings
from .layers import GPLayer, LatentVariableLayer, RegularizerType
from .likelihoods import is_gaussian, output_dim, predictive_dim, target_dim
from .temp_workaround import draw_normal, precompute_states


def _data(x):
    t = torch.as_tensor(np.asarray(x, dtype=np.float32) if not isinstance(x, torch.Tensor) else x)
    return t.to(dtype=settings.float_type, device=settings.default_device()).contiguous()


class Bound:
    """A member of the bound family between the K-sample ELBO and the importance-weighted bound (include/iwvi_hip.h: iwvi_bound_desc;
    Rainforth et al. 2018, Li & Turner 2016).  Per data point, with the K samples in ``groups`` contiguous groups of K / groups:

        bound_n = beta mean_k L_nk + (1 - beta) mean_g (1 / (1 - alpha)) [logsumexp_{k in g}((1 - alpha) L_nk) - log(K / groups)]

    ``Bound.iwae()`` = (1, 0, 0) is the importance-weighted bound; ``miwae(groups)`` averages the groups' bounds, ``ciwae(beta)`` mixes the
    ELBO in, ``vr(alpha)`` tempers the log-sum-exp.  ``parse`` reads "iwae" | "miwae:4" | "ciwae:0.5" | "vr:0.3", a "+"-joined combination
    of them, and the ``repr`` of a Bound."""
    __slots__ = ("groups", "alpha", "beta")

    def __init__(self, groups=1, alpha=0.0, beta=0.0):
        if isinstance(groups, bool) or int(groups) != groups or int(groups) < 1:
            raise ValueError("Bound: groups must be an integer >= 1 (and divide num_samples), got %r" % (groups,))
        alpha, beta = float(alpha), float(beta)
        if not 0.0 <= alpha < 1.0 or not np.float32(1.0 - alpha) > 0:
            raise ValueError("Bound: alpha must lie in [0, 1) (tau = 1 - alpha in (0, 1]), got %r" % (alpha,))
        if not 0.0 <= beta <= 1.0:
            raise ValueError("Bound: beta must lie in [0, 1], got %r" % (beta,))
        object.__setattr__(self, "groups", int(groups))
        object.__setattr__(self, "alpha", alpha)
        object.__setattr__(self, "beta", beta)

    def __setattr__(self, name, value):
        raise AttributeError("a Bound is immutable: assign a new one to model.bound")

    @classmethod
    def iwae(cls):
        return cls()

    @classmethod
    def miwae(cls, groups):
        return cls(groups=groups)

    @classmethod
    def ciwae(cls, beta):
        return cls(beta=beta)

    @classmethod
    def vr(cls, alpha):
        return cls(alpha=alpha)

    @classmethod
    def parse(cls, text):
        if isinstance(text, cls):
            return text
        if not isinstance(text, str):
            raise ValueError("Bound.parse reads a string such as 'iwae', 'miwae:4', 'ciwae:0.5' or 'vr:0.3', got %r" % (text,))
        s = text.strip()
        if s.startswith("Bound.parse(") and s.endswith(")"):
            s = s[len("Bound.parse("):-1].strip().strip("'\"")
        kw = {}
        for part in s.split("+"):
            name, _, arg = part.strip().partition(":")
            try:
                if name == "iwae" and not arg:
                    continue
                key, val = {"miwae": ("groups", int), "ciwae": ("beta", float), "vr": ("alpha", float)}[name]
                if key in kw:
                    raise KeyError(name)
                kw[key] = val(arg)
            except (KeyError, ValueError):
                raise ValueError("Bound.parse: %r is not 'iwae', 'miwae:<groups>', 'ciwae:<beta>' or 'vr:<alpha>' (or several joined by '+')"
                                 % (text,)) from None
        return cls(**kw)

    @property
    def tau(self):
        return 1.0 - self.alpha

    @property
    def is_default(self):
        return self.groups == 1 and self.alpha == 0.0 and self.beta == 0.0

    def _key(self):
        return (self.groups, self.alpha, self.beta)

    def __eq__(self, other):
        return isinstance(other, Bound) and self._key() == other._key()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self._key())

    def __str__(self):
        parts = (["miwae:%d" % self.groups] if self.groups != 1 else []) + (["ciwae:%r" % self.beta] if self.beta else []) + \
                (["vr:%r" % self.alpha] if self.alpha else [])
        return "+".join(parts) or "iwae"

    def __repr__(self):
        return "Bound.parse(%r)" % str(self)

    def check_samples(self, K):
        """The point of use: the groups divide the model's K."""
        if K % self.groups:
            raise ValueError("bound %s: groups=%d does not divide num_samples=%d" % (self, self.groups, K))

    def desc(self):
        d = _abi.BoundDesc()
        d.groups, d.tau, d.beta = self.groups, self.tau, self.beta
        return d


class DGP_VI:
    def __init__(self, X, Y, layers, likelihood, num_samples=1, minibatch_size=None, name=None):
        self.likelihood = likelihood
        if hasattr(likelihood, "check_targets"):                      # (a Bernoulli refuses labels other than 0 / 1 here, once, on the host)
            likelihood.check_targets(Y)
        self.layers = list(layers)
        if hasattr(likelihood, "check_output_dim"):                   # (MultiClass: one output per class; HeteroskedasticGaussian: an even number)
            likelihood.check_output_dim(self._output_dim() if self.layers else None)
        self.num_data = X.shape[0]                                    # models.py:18
        self.num_samples = num_samples
        self._X_all, self._Y_all = _data(X), _data(Y)
        self.minibatch_size = minibatch_size
        self._mb_rng = np.random.RandomState(0)                       # Minibatch(seed=0), models.py:25-26
        self._mb_perm, self._mb_pos = None, 0
        self._mb_serial = 0                                           # bumped by every minibatch change: cache key
        self.X, self.Y = self._X_all, self._Y_all
        if minibatch_size is not None:
            self.next_minibatch()
        self.name = name
        self.full_cov_over_samples = False
        # IW-ELBO only: evaluate a leading latent-variable layer inside the precompute launch (beside the
        # factorisations) instead of inside the layer kernel; keep_lv_noise exports its draws (tests)
        self.lv_in_precompute = False
        self.keep_lv_noise = False
        self._dev_words = None

    # -- lv_in_precompute: refused when it is switched on, not at the first evaluation, for an encoder the precompute launch cannot hold --
    @property
    def lv_in_precompute(self):
        return self._lv_in_precompute

    @lv_in_precompute.setter
    def lv_in_precompute(self, on):
        if on and self.layers and isinstance(self.layers[0], LatentVariableLayer):
            why = self.layers[0].precompute_refusal()
            if why:
                raise ValueError(why)
        self._lv_in_precompute = bool(on)

    # -- the estimator of the encoder gradient (configuration, not state: no checkpoint carries it) ------------
    # "iwae": the reparameterised gradient of the bound; "dreg" / "stl": the doubly reparameterised estimator and "sticking the landing"
    # (include/iwvi_hip.h: IWVI_LV_GRAD_*), which exist for the sampled regulariser of DGP_IWVI only
    ENCODER_GRADIENTS = ("iwae",)
    _encoder_gradient = "iwae"

    @property
    def encoder_gradient(self):
        return self._encoder_gradient

    @encoder_gradient.setter
    def encoder_gradient(self, name):
        if name not in self.ENCODER_GRADIENTS:
            raise ValueError("%s.encoder_gradient is one of %s, not %r" % (type(self).__name__, " | ".join(self.ENCODER_GRADIENTS), name))
        self._encoder_gradient = name

    # -- the bound (configuration, as the estimator above): DGP_IWVI alone has the family; the analytic-KL bound of this class is its own --
    BOUND_FAMILY = False
    _bound = Bound()

    @property
    def bound(self):
        return self._bound

    @bound.setter
    def bound(self, value):
        value = Bound.parse(value)
        if not value.is_default and not self.BOUND_FAMILY:
            raise ValueError("%s.bound: the bound family (%s) belongs to the importance-weighted DGP_IWVI; the analytic-KL bound of "
                             "DGP_VI has the default only" % (type(self).__name__, value))
        self._bound = value

    # -- data ---------------------------------------------------------------------------------
    def next_minibatch(self):
        """Advance to the next minibatch (shuffled epochs, X and Y aligned like gpflow.Minibatch)."""
        if self.minibatch_size is None:
            return
        n = self._X_all.shape[0]          # the rows THIS model holds (num_data may be the job total of a data-parallel run)
        b = min(self.minibatch_size, n)
        if self._mb_perm is None or self._mb_pos + b > n:
            self._mb_perm = torch.as_tensor(self._mb_rng.permutation(n), device=self._X_all.device)
            self._mb_pos = 0
        idx = self._mb_perm[self._mb_pos:self._mb_pos + b]
        self._mb_pos += b
        if self.X.shape[0] == b and self.X.data_ptr() != self._X_all.data_ptr():
            # same buffers every step (a captured hipGraph of the step keeps reading them)
            torch.index_select(self._X_all, 0, idx, out=self.X)
            torch.index_select(self._Y_all, 0, idx, out=self.Y)
        else:
            self.X, self.Y = self._X_all[idx].contiguous(), self._Y_all[idx].contiguous()
        self._mb_serial += 1         # the caching allocator reuses addresses: pointers alone cannot key the per-minibatch caches

    def to(self, device):
        self._X_all, self._Y_all = self._X_all.to(device), self._Y_all.to(device)
        self.X, self.Y = self.X.to(device), self.Y.to(device)
        self._mb_serial += 1
        for layer in self.layers:
            layer.to(device)
        if hasattr(self.likelihood, "to"):                            # (an Ordinal's device buffer [sigma, edges])
            self.likelihood.to(device)
        return self

    def _words(self):
        """[ticket, rng step, rng ticket, draw serial] device words, zeroed once (never per call).  Word 3 belongs to ``predict_y_draws``
        (``iwvi_lik_sample_y``'s ``serial_dev``): the serial in its low half, the running launch's arrival count in its high half."""
        dev = self.X.device
        if self._dev_words is None or self._dev_words.device != dev:
            self._dev_words = torch.zeros(4, dtype=torch.int64, device=dev)
        return self._dev_words

    # -- reference API ------------------------------------------------------------------------
    def precompute(self, with_encoders=False, sample_first=None, dense=False, q_moved=None):
        """Gram + Cholesky + operand packing of every GP layer: one ABI call, one launch.  ``with_encoders``:
        the same launch also evaluates the encoder MLP of every latent-variable layer on the current minibatch
        (it does not depend on the factorisation, so it runs beside it instead of inside the layer kernel).
        ``sample_first`` = dict(K, sampled_kl, want_z): a latent-variable layer at position 0 is evaluated in full
        there (its K samples per row, their regulariser); ``_fused_forward(stack_from=1)`` continues from it."""
        encs, keep = [], []
        if with_encoders:
            for i, l in enumerate(self.layers):
                if isinstance(l, LatentVariableLayer) and len(encs) < 2:
                    smp = None
                    if sample_first is not None and i == 0:
                        smp = dict(sample_first, X=self.X, layer_index=0, seed=settings.seed,
                                   rng_state=ctypes.c_void_p(self._words().data_ptr() + 8))
                    e, k = l.enc_desc(self._xy_minibatch(), sample=smp)
                    if e is not None:                            # (None: a custom-activation encoder, already evaluated by torch ops)
                        encs.append(e)
                    keep.append(k)
                    l._enc_key = self._mb_key()
        if q_moved is None:
            descs = [l.state_desc() for l in self.layers if isinstance(l, GPLayer)]
        else:
            # ``q_moved`` (layer indices; the CALLER vouches for it -- training.Trainer.step between its two ops): since the last full precompute
            # on these state buffers nothing but these layers' q(u) has changed.  Their q(u) images are rewritten (IWVI_GP_REUSE_FACTOR), every
            # factorisation stays as it is, a layer of which nothing moved is not in the call at all; the encoders run as always.
            descs = []
            for i in sorted(q_moved):
                d = self.layers[i].state_desc()
                d.flags |= _abi.GP_REUSE_FACTOR
                descs.append(d)
            if dense or not descs:
                raise ValueError("q_moved: at least one layer, and not together with dense")
        if dense:                                                    # the adjoints read the dense float64 Lm, Lm^-1
            for d in descs:                                          # ("lm": the factor only; Lm^-1 by iwvi_gp_dense_inverse)
                d.flags |= _abi.GP_WANT_LM if dense == "lm" else _abi.GP_WANT_DENSE
        precompute_states(descs, encs)
        if dense == "lm" and descs:
            arr = (_abi.GpDesc * len(descs))(*descs)
            _abi.check(_abi.lib().iwvi_gp_dense_inverse(arr, len(descs), _abi.stream_ptr()))

    def autotune_f64(self, threshold=300.0):
        """Record every GP layer's MEASURED float64-route choice from the factor itself: max / min of diag(Lm) of the CURRENT parameters
        (one precompute launch with the dense factors for all layers + ONE read-back: a synchronisation, so it is a calibration call -- after
        building or loading a model, at every staircase epoch of a training run (``training.Trainer`` does both) -- not part of an evaluation).
        diag(Lm) spans [sqrt(jitter), sigma] -- at most 1e3 at the default jitter and unit variance.  Measured (scripts/diag_ratio.py): 14 / 28 / 85
        at the BASELINE stacks (8-D, M = 128 / 256 / 512), 430 at 4-D M = 128, 820-990 for 1-3-D inputs at any M >= 32; the default
        ``threshold`` 300 separates what float32 holds at the stated tolerance from what it does not (profiles/r05_f64_route_error.txt).
        A layer's explicit ``f64_stage1 = True / False`` still wins over the measurement.  Returns [{layer, diag_ratio, f64_stage1}]."""
        gps = [(i, l) for i, l in enumerate(self.layers) if isinstance(l, GPLayer)]
        self.precompute(dense=True)
        ratios = []
        for _, l in gps:
            st = l.state()
            d = torch.diagonal(st.view("Lm", torch.float64, st.Mp * st.Mp).view(st.Mp, st.Mp)[:st.M, :st.M])
            ratios.append(d.max() / d.min())
        ratios = torch.stack(ratios).tolist() if ratios else []    # the one device-to-host copy
        rep = []
        for (i, l), ratio in zip(gps, ratios):
            l._f64_measured = bool(ratio >= threshold) if ratio == ratio else True      # (NaN: the float32 image of the factor broke down)
            rep.append(dict(layer=i, diag_ratio=float(ratio), f64_stage1=l.uses_f64_stage1()))
        self.precompute()                                         # (the states as an evaluation expects them: flags of the new choice)
        return rep

    def route_key(self):
        """What a captured graph bakes in besides the shapes: each GP layer's arithmetic route (``training.Trainer`` re-captures when it moves)."""
        return tuple((l.uses_f64_stage1(), bool(settings.fw_f32_stage2)) for l in self.layers if isinstance(l, GPLayer))

    def propagate(self, X, full_cov=False, inference_amorization_inputs=None,
                  is_sampled_local_regularizer=False, zs=None, _precomputed=False, _kl_parts=False, _last_sample=True):
        """reference models.py:31-46 -> (samples[1:], means, covs, kls, kl_types); one launch per layer.
        ``_last_sample=False``: the final layer's sample is not needed (None is returned in its place)."""
        if not _precomputed:
            self.precompute()
        samples, means, covs, kls, kl_types = [X, ], [], [], [], []
        zs = [None] * len(self.layers) if zs is None else zs
        if len(zs) != len(self.layers):
            raise ValueError("zs needs one entry per layer")
        for i, (layer, z) in enumerate(zip(self.layers, zs)):
            sample, mean, cov, kl = layer.propagate(samples[-1], full_cov=full_cov,
                                                    inference_amorization_inputs=inference_amorization_inputs,
                                                    is_sampled_local_regularizer=is_sampled_local_regularizer,
                                                    z=z, _precomputed=True, _kl_parts=_kl_parts,
                                                    _want_sample=_last_sample or i + 1 < len(self.layers))
            samples.append(sample)
            means.append(mean)
            covs.append(cov)
            kls.append(kl)
            kl_types.append(layer.regularizer_type)
        return samples[1:], means, covs, kls, kl_types

    # -- fused forward ------------------------------------------------------------------------
    def _fused_forward(self, T, row_div, row_mod, lead, zs=None, sampled_kl=True, want_layers=False,
                       want_logw=True, use_encoder=True, elbo=None, stack_from=0, want_saved=False, outputs_for=None, moments=True,
                       X=None, Y=None, predict=None, local_kls=False):
        """``iwvi_dgp_forward`` over the current minibatch: every layer + log-weights in one launch.
        Row t of the flattened batch reads data row (t // row_div) % row_mod.  ``elbo`` = dict(B, K, stride_b,
        stride_k, mode_vi, want_ms, K_total): also run the reduction of models.py:138-150 in the tail of the
        launch.  Returns (logw [T] or None, per-layer dict lists when ``want_layers``, (elbo, logp, ms) or None).
        ``stack_from=1`` (needs ``elbo``): layer 0 was evaluated by ``precompute(sample_first=...)``; the launch
        starts from its samples [T, Dx+Lw] and its per-sample regulariser.
        ``outputs_for`` (with ``want_layers``): only these layers (indices into the stack) get output buffers, the others write
        nothing; ``moments=False``: no sample / mean / var rows either (only what ``want_saved`` adds) -- the natural-gradient op needs
        the final layer's a, noise and latent moments alone.
        ``X`` / ``Y``: explicit inputs and targets in place of the current minibatch.  ``predict`` = dict(S, out): run
        ``iwvi_dgp_predict_density`` instead (rows t = n S + s, latent-variable layers in prior mode: ``use_encoder=False``),
        writing the per-point Monte Carlo log predictive density into ``out`` [N]; ``predict`` = dict(S, out_y[, z_y]): run
        ``iwvi_dgp_predict_samples`` -- the same rows, y samples into ``out_y`` [N, S, Dy] (``z_y`` [N S, Dy]: the likelihood's noise).
        ``local_kls`` (with ``outputs_for``): a latent-variable layer outside ``outputs_for`` still writes its regulariser (nothing else).
        The tail of the launch (``want_logw`` with targets, ``elbo``, ``predict``) is Gaussian: other likelihoods call it without one."""
        dev = self.X.device
        gauss = is_gaussian(self.likelihood)
        if not gauss and (want_logw or elbo is not None or predict is not None):
            raise NotImplementedError("the fused tail of iwvi_dgp_forward is Gaussian; %s goes through the layer launch + iwvi_lik_elbo_reduce"
                                      % type(self.likelihood).__name__)
        lik_host, lik_dev = self.likelihood.desc_variance() if gauss else (1.0, None)
        layers = self.layers[stack_from:]
        n = len(layers)
        if n > _abi.MAX_STACK:
            raise ValueError("more than %d layers in one fused launch" % _abi.MAX_STACK)
        zs = [None] * n if zs is None else zs
        if len(zs) != n:
            raise ValueError("zs needs one entry per layer")
        if stack_from:
            first = self.layers[0]
            if stack_from != 1 or elbo is None or getattr(first, "_smp_X", None) is None or first._smp_X.shape[0] != T:
                raise ValueError("stack_from=1 needs elbo and precompute(sample_first=...) on this minibatch")
            X = first._smp_X
        else:
            X = _abi.dev_tensor((self.X if X is None else X).contiguous(), "X")
        Y = _abi.dev_tensor((self.Y if Y is None else Y).contiguous(), "Y")
        XY = self._xy_minibatch() if use_encoder and any(isinstance(l, LatentVariableLayer) for l in layers) else None
        descs = (_abi.LayerDesc * n)()
        keep, outs = [], []
        D = X.shape[1]
        for i, (layer, z) in enumerate(zip(layers, zs)):
            if isinstance(layer, GPLayer):
                R = layer.num_outputs
                z2 = None if z is None else _abi.dev_tensor(z.reshape(T, R).contiguous(), "z")
                o = None
                if want_layers and (outputs_for is None or i in outputs_for):
                    P = layer.kern.W.shape[0] if hasattr(layer.kern, "W") else R
                    o = {k: torch.empty(*lead, P, dtype=settings.float_type, device=dev) for k in ("sample", "mean", "var")} if moments else {}
                    if want_saved:                               # what the adjoint of this layer needs (backward.py)
                        Mp = layer.state().Mp
                        o["a_out"] = torch.empty(T, Mp, dtype=settings.float_type, device=dev)
                        from .backward import needs_saved_u
                        if needs_saved_u(layer, T):     # only the GEMM path of the adjoint reads u_r = L_r^T a
                            o["u_out"] = torch.empty(R, T, Mp, dtype=settings.float_type, device=dev)
                        o["noise_out"] = torch.empty(T, R, dtype=settings.float_type, device=dev)
                        o["gmv_out"] = torch.empty(T, 3 * R, dtype=settings.float_type, device=dev)
                d, k = layer.fused_desc(z2, o)
                if d.D != D:
                    raise ValueError("layer %d expects %d inputs, got %d" % (i, d.D, D))
                D = d.P
            elif isinstance(layer, LatentVariableLayer):
                Lw = layer.latent_dim
                z2 = None if z is None else _abi.dev_tensor(z.reshape(T, Lw).contiguous(), "z")
                o = None
                listed = outputs_for is None or i in outputs_for
                if want_layers and (listed or local_kls):
                    o = {k: torch.empty(*lead, D + Lw, dtype=settings.float_type, device=dev) for k in ("sample", "mean", "var")} if (moments and listed) else {}
                    o["kl_local"] = torch.empty(*lead, Lw, dtype=settings.float_type, device=dev)
                    if want_saved and listed:
                        o["noise_out"] = torch.empty(T, Lw, dtype=settings.float_type, device=dev)
                # encoder output of THIS minibatch from the last precompute launch, if there is one
                eo = layer._enc_out if (use_encoder and getattr(layer, "_enc_key", None) == self._mb_key()) else None
                if eo is None and use_encoder and layer.encoder.custom_act is not None:      # a custom activation never runs inside the kernels
                    layer.enc_desc(self._xy_minibatch())
                    layer._enc_key = self._mb_key()
                    eo = layer._enc_out
                d, k = layer.fused_desc(D, z2, o, sampled_kl=sampled_kl, use_encoder=use_encoder, enc_out=eo)
                D += Lw
            else:
                raise TypeError("the fused forward knows GPLayer and LatentVariableLayer; use propagate() for custom layers")
            descs[i] = d
            keep.append(k)
            outs.append(o)
        words = self._words()
        if predict is not None and "out_y" in predict:
            N, S, out_y, z_y = X.shape[0], predict["S"], predict["out_y"], predict.get("z_y")
            _abi.check(_abi.lib().iwvi_dgp_predict_samples(descs, n, _abi.ptr(X), X.shape[1], out_y.shape[-1], N, S, lik_host, lik_dev,
                                                           _abi.ptr(z_y), settings.seed, ctypes.c_void_p(words.data_ptr() + 8),
                                                           _abi.ptr(out_y), _abi.stream_ptr()))
            return None, outs, None
        if predict is not None:
            N, S, out = X.shape[0], predict["S"], predict["out"]
            ws = torch.empty((_abi.lib().iwvi_dgp_predict_density_ws_bytes(N, S) + 3) // 4, dtype=torch.float32, device=dev)
            _abi.check(_abi.lib().iwvi_dgp_predict_density(descs, n, _abi.ptr(X), X.shape[1], _abi.ptr(Y), Y.shape[1], N, S,
                                                           lik_host, lik_dev, settings.seed, ctypes.c_void_p(words.data_ptr() + 8),
                                                           _abi.ptr(out), _abi.ptr(ws), _abi.stream_ptr()))
            return None, outs, None
        logw = torch.empty(T, dtype=settings.float_type, device=dev) if want_logw else None
        ed, red = None, None
        if elbo is not None:
            B, K = elbo["B"], elbo["K"]
            glob = [_abi.dev_tensor(g.reshape(-1), "global kl", torch.float64) for g in self._global_kls()]
            glob_p = _abi.ptr_array(glob)
            glob_n = (ctypes.c_int32 * max(len(glob), 1))(*[g.numel() for g in glob])
            logp = torch.empty(B, dtype=settings.float_type, device=dev)
            # caller-provided result buffers (e.g. a slot of an exchange staging ring) or fresh ones
            val = elbo.get("elbo_out")
            val = torch.empty(1, dtype=torch.float64, device=dev) if val is None else _abi.dev_tensor(val.view(-1), "elbo_out", torch.float64)
            ms = elbo.get("ms_out")
            if ms is not None:
                ms = _abi.dev_tensor(ms, "ms_out", settings.float_type)
                if tuple(ms.shape) != (B, 2):
                    raise ValueError("ms_out must be [B, 2]")
            elif elbo.get("want_ms"):
                ms = torch.empty(B, 2, dtype=settings.float_type, device=dev)
            ed = _abi.ElboDesc()
            ed.B, ed.K, ed.stride_b, ed.stride_k = B, K, elbo["stride_b"], elbo["stride_k"]
            ed.kl_global, ed.kl_global_counts, ed.n_glob = glob_p, glob_n, len(glob)
            ed.scale = float(self.num_data) / float(B)                     # models.py:80-81, :144-145
            ed.K_total, ed.mode_vi = elbo.get("K_total") or K, 1 if elbo["mode_vi"] else 0
            ed.out_lse_ms = None if ms is None else ms.data_ptr()
            ed.lik_variance_dev = lik_dev
            ws = torch.empty((T + 15) // 16, dtype=torch.float64, device=dev)
            ed.out_logp, ed.out_elbo, ed.ws = logp.data_ptr(), val.data_ptr(), ws.data_ptr()
            adj = elbo.get("adj")                                # heads of the bound's adjoint from the same launch (backward.py)
            if adj is not None:
                ed.adj_w, ed.adj_dmean, ed.adj_dvar, ed.adj_sums = (adj["w"].data_ptr(), adj["d_mean"].data_ptr(),
                                                                    adj["d_var"].data_ptr(), adj["sums"].data_ptr())
            if stack_from:
                ed.lw_init, ed.noise_layer_base, ed.x_per_sample = self.layers[0]._smp_kl.data_ptr(), stack_from, 1
            keep.append((glob, glob_p, glob_n, ws))
            red = (val[0], logp, ms)
        args = (descs, n, _abi.ptr(X), X.shape[1], _abi.ptr(XY), 0 if XY is None else XY.shape[1],
                _abi.ptr(Y) if want_logw else None, Y.shape[1], T, row_div, row_mod,
                lik_host if (ed is not None or not want_logw) else self.likelihood.variance,
                settings.seed, ctypes.c_void_p(words.data_ptr() + 8), _abi.ptr(logw),
                None if ed is None else ctypes.byref(ed), _abi.stream_ptr())
        _abi.check(_abi.lib().iwvi_dgp_forward(*args))
        return logw, outs, red

    def _mb_key(self):
        return (self._mb_serial, self.X.data_ptr(), self.Y.data_ptr(), self.X.shape[0])

    def invalidate_minibatch_caches(self):
        """Call after changing ``model.X`` / ``model.Y`` IN PLACE (the [x, y] rows and encoder outputs are cached per minibatch)."""
        self._mb_serial += 1

    def _xy_minibatch(self):
        """[x_b, y_b] rows of the current minibatch (models.py:53 / :116 before tiling), cached per minibatch."""
        key = self._mb_key()
        if getattr(self, "_xy_key", None) != key:
            cur = getattr(self, "_xy_cache", None)
            shape = (self.X.shape[0], self.X.shape[1] + self.Y.shape[1])
            if cur is not None and tuple(cur.shape) == shape and cur.device == self.X.device:
                torch.cat([self.X, self.Y], -1, out=cur)          # same buffer every minibatch (graph capture)
            else:
                self._xy_cache = torch.cat([self.X, self.Y], -1).contiguous()
            self._xy_key = key
        return self._xy_cache

    def _global_kls(self):
        # (a GP layer without q_sqrt -- the SGHMC mode -- hands over the negative log prior of its q_mu instead of the state's KL shares)
        return [l.global_regulariser_parts() if isinstance(l, GPLayer) else l.state().kl_parts
                for l in self.layers if l.regularizer_type is RegularizerType.GLOBAL]

    def _reduce_logw(self, logw, global_kls, B, K, stride_b, stride_k, mode_vi, want_ms=False, K_total=None):
        """``iwvi_logw_reduce``: logsumexp/mean over K + scaled sum - global KLs (models.py:138-150, :69-86)."""
        dev = logw.device
        glob = [_abi.dev_tensor(g.reshape(-1), "global kl", torch.float64) for g in global_kls]
        glob_n = (ctypes.c_int32 * max(len(glob), 1))(*[g.numel() for g in glob])
        logp = torch.empty(B, dtype=settings.float_type, device=dev)
        elbo = torch.empty(1, dtype=torch.float64, device=dev)
        ms = torch.empty(B, 2, dtype=settings.float_type, device=dev) if want_ms else None
        scale = float(self.num_data) / float(B)                        # models.py:80-81, :144-145
        _abi.check(_abi.lib().iwvi_logw_reduce(
            _abi.ptr(logw), B, K, stride_b, stride_k, _abi.ptr_array(glob), glob_n, len(glob),
            scale, K_total or K, 1 if mode_vi else 0, _abi.ptr(ms), _abi.ptr(logp), _abi.ptr(elbo),
            _abi.ptr(self._words()), _abi.stream_ptr()))
        return elbo[0], logp, ms

    def _reduce(self, fmean, fvar, Y, local_kls, global_kls, B, K, stride_b, stride_k, mode_vi,
                want_ms=False, K_total=None, ms_out=None, elbo_out=None):
        """``iwvi_iw_elbo_reduce`` on explicit final-layer moments (the layer-by-layer path)."""
        dev = fmean.device
        Dy = output_dim(self.likelihood, Y.shape[-1])                # (MultiClass: Y is one column of labels, the moments have C; hetero: 2 per column)
        fmean = _abi.dev_tensor(fmean.contiguous(), "final mean")
        fvar = _abi.dev_tensor(fvar.contiguous(), "final var")
        Y = _abi.dev_tensor(Y.contiguous(), "Y")
        kls = [_abi.dev_tensor(k.contiguous(), "local kl") for k in local_kls]
        if len(kls) > _abi.MAX_KL:
            raise ValueError("more than %d latent-variable layers" % _abi.MAX_KL)
        kl_dims = (ctypes.c_int32 * max(len(kls), 1))(*[k.shape[-1] for k in kls])
        glob = [_abi.dev_tensor(g.reshape(-1), "global kl", torch.float64) for g in global_kls]
        glob_n = (ctypes.c_int32 * max(len(glob), 1))(*[g.numel() for g in glob])
        logp = torch.empty(B, dtype=settings.float_type, device=dev)
        elbo = torch.empty(1, dtype=torch.float64, device=dev)
        ms = torch.empty(B, 2, dtype=settings.float_type, device=dev) if (want_ms and ms_out is None) else None
        scale = float(self.num_data) / float(B)                        # models.py:80-81, :144-145
        # (a trained likelihood variance is read on the device: no device-to-host copy here -- there must be none inside a captured step --
        #  and a replayed graph follows the value)
        if not is_gaussian(self.likelihood):                            # the same reduction with the likelihood's own expectation
            if ms_out is not None:
                ms = _abi.dev_tensor(ms_out, "ms_out", settings.float_type)
                if tuple(ms.shape) != (B, 2):
                    raise ValueError("ms_out must be [B, 2]")
            if elbo_out is not None:
                elbo = _abi.dev_tensor(elbo_out.view(-1), "elbo_out", torch.float64)
            _abi.check(_abi.lib().iwvi_lik_elbo_reduce(
                self.likelihood.lik_desc(), _abi.ptr(fmean), _abi.ptr(fvar), _abi.ptr(Y), B, K, Dy,
                stride_b, stride_k, _abi.ptr_array(kls), kl_dims, len(kls), _abi.ptr_array(glob), glob_n, len(glob),
                scale, K_total or K, 1 if mode_vi else 0, _abi.ptr(ms), _abi.ptr(logp), _abi.ptr(elbo),
                _abi.ptr(self._words()), _abi.stream_ptr()))
            return elbo[0], logp, ms
        lik_host, lik_dev = self.likelihood.desc_variance()
        _abi.check(_abi.lib().iwvi_iw_elbo_reduce_dev(
            _abi.ptr(fmean), _abi.ptr(fvar), _abi.ptr(Y), lik_host, lik_dev, B, K, Dy,
            stride_b, stride_k, _abi.ptr_array(kls), kl_dims, len(kls), _abi.ptr_array(glob), glob_n, len(glob),
            scale, K_total or K, 1 if mode_vi else 0, _abi.ptr(ms), _abi.ptr(logp), _abi.ptr(elbo),
            _abi.ptr(self._words()), _abi.stream_ptr()))
        return elbo[0], logp, ms

    def _moments_then_reduce(self, T, row_div, row_mod, lead, zs, sampled_kl, red):
        """A likelihood without a fused tail (the caller has run ``precompute``): the layer launch leaves the final layer's moments and every
        local regulariser -- nothing else reaches memory --, ``_reduce(**red)`` finishes (``iwvi_lik_elbo_reduce``)."""
        last = len(self.layers) - 1
        _, outs, _ = self._fused_forward(T, row_div, row_mod, lead, zs=zs, sampled_kl=sampled_kl, want_layers=True, want_logw=False,
                                         outputs_for={last}, local_kls=True)
        local_kls = [o["kl_local"].reshape(T, -1) for o, l in zip(outs, self.layers) if l.regularizer_type is RegularizerType.LOCAL]
        return self._reduce(outs[last]["mean"].reshape(T, -1), outs[last]["var"].reshape(T, -1), self.Y, local_kls, self._global_kls(), **red)

    def _build_likelihood(self, zs=None):
        """The VI bound, reference models.py:49-86 (2-D [S*N, D] tiling, mean over S)."""
        S, N = self.num_samples, self.X.shape[0]
        self.precompute(with_encoders=True)
        if not is_gaussian(self.likelihood):
            return self._moments_then_reduce(S * N, 1, N, (S * N,), zs, False,
                                             dict(B=N, K=S, stride_b=1, stride_k=N, mode_vi=True))[0]
        # tile(X, [S, 1]) (:50-53): row t = s*N + n reads data row t % N; analytic local KL (:58-61)
        _, _, red = self._fused_forward(S * N, 1, N, (S * N,), zs=zs, sampled_kl=False,
                                        elbo=dict(B=N, K=S, stride_b=1, stride_k=N, mode_vi=True))
        return red[0]

    def compute_log_likelihood(self, zs=None):
        """gpflow ``Model.compute_log_likelihood`` (reference tests/test_gp_layer.py:50): host float."""
        return float(self._build_likelihood(zs).item())

    likelihood_tensor = property(lambda self: self._build_likelihood())

    def _build_predict(self, X, full_cov=False, zs=None):
        _, means, covs, _, _ = self.propagate(X, full_cov=full_cov, zs=zs, _last_sample=False)   # :89-91
        return means[-1], covs[-1]

    def predict_f(self, X, zs=None):
        return self._build_predict(_data(X), False, zs)

    def predict_f_full_cov(self, X, zs=None):
        return self._build_predict(_data(X), True, zs)

    def predict_f_multisample(self, X, S, zs=None):
        X = _data(X)
        X_tiled = X[None, :, :].expand(S, *X.shape).contiguous()       # :97
        _, means, covs, _, _ = self.propagate(X_tiled, zs=zs)
        return means[-1], covs[-1]

    def predict_y(self, X, zs=None):
        """gpflow ``GPModel.predict_y``: the likelihood's predictive mean and variance at one draw through the inner layers."""
        return self.likelihood.predict_mean_and_var(*self._build_predict(_data(X), False, zs))

    def predict_density(self, X, Y, zs=None):
        """gpflow ``GPModel.predict_density``: log N(Y; m, v + variance) [N, Dy] at one draw through the inner layers."""
        X = _data(X)
        Y = _data(Y)
        return self.likelihood.predict_density(*self._build_predict(X, False, zs), Y)

    def _input_dim(self):
        """Columns of X the stack expects: the first GP layer's input width less the latent dimensions added in front of it."""
        lat = 0
        for l in self.layers:
            if isinstance(l, GPLayer):
                return l._Z().shape[1] - lat
            lat += l.latent_dim
        return None

    def _output_dim(self):
        last = self.layers[-1]
        if not isinstance(last, GPLayer):
            return None
        return last.kern.W.shape[0] if hasattr(last.kern, "W") else last.num_outputs

    _PREDICT_ROWS = 1 << 24                          # default cap on N x S rows per launch (the forward takes < 2^31)

    def predict_log_density(self, X, Y, S, zs=None, batch_size=None):
        """Monte Carlo log predictive density [N]: log (1/S) sum_s prod_d N(y_nd; m_snd, v_snd + variance), the final layer's moments of
        S draws through the inner layers (drawn as in ``predict_f_multisample``; ``zs``: one [S, N, dim] array or None per layer).  One
        precompute, then per batch of ``batch_size`` points one ``iwvi_dgp_predict_density`` call (the fused forward with a predictive
        tail, and the merge of its per-point partials): no per-layer sample, moment or log-weight reaches memory.  A likelihood other than
        the Gaussian: ``predict_mixture(X, S, Y)["log_density"]`` -- sum_d of ITS predict_density in place of the Gaussian's."""
        X, Y = _data(X), _data(Y)
        S = int(S)
        if S < 1:
            raise ValueError("S must be >= 1, got %d" % S)
        if X.dim() != 2 or X.shape[1] != self._input_dim():
            raise ValueError("X must be [N, %s], got %s" % (self._input_dim(), tuple(X.shape)))
        Dy = self._output_dim()
        Yd = target_dim(self.likelihood, Dy)
        if Y.dim() != 2 or Y.shape[0] != X.shape[0] or Y.shape[1] != Yd:
            raise ValueError("Y must be [%d, %s], got %s" % (X.shape[0], Yd, tuple(Y.shape)))
        N = X.shape[0]
        if not is_gaussian(self.likelihood):                         # three launches per batch: precompute, layers, iwvi_lik_predict_mixture
            return self.predict_mixture(X, S, Y=Y, zs=zs, batch_size=batch_size, _moments=False)["log_density"]
        zs = self._check_predict_noise("predict_log_density", S, N, zs)
        bs = batch_size or max(1, self._PREDICT_ROWS // S)
        if bs < 1:
            raise ValueError("batch_size must be >= 1")
        out = torch.empty(N, dtype=settings.float_type, device=X.device)
        if N == 0:
            return out
        self.precompute()
        for lo in range(0, N, bs):
            hi = min(N, lo + bs)
            nb = hi - lo
            zb = [None if z is None else _data(z)[:, lo:hi].transpose(0, 1).reshape(nb * S, -1) for z in zs]   # point-major rows n S + s
            self._fused_forward(nb * S, S, nb, (nb * S,), zs=zb, want_logw=False, use_encoder=False,
                                X=X[lo:hi], Y=Y[lo:hi], predict=dict(S=S, out=out[lo:hi]))
        return out

    def _predict_log_density_layerwise(self, X, Y, S, zs=None, batch_size=None):
        """``predict_log_density`` of a non-Gaussian likelihood as it ran before ``predict_mixture`` existed, kept as the route the tests and
        scripts/time_predict_mixture.py compare with: per batch the layer-by-layer launches of ``predict_f_multisample``, Y expanded to
        [S, N, .], one elementwise ``iwvi_lik_predict_density`` launch, then a torch ``logsumexp``."""
        X, Y = _data(X), _data(Y)
        S, N = int(S), X.shape[0]
        zs = self._check_predict_noise("predict_log_density", S, N, zs)
        bs = int(batch_size or max(N, 1))
        if bs < 1:
            raise ValueError("batch_size must be >= 1")
        out = torch.empty(N, dtype=settings.float_type, device=X.device)
        for lo in range(0, N, bs):
            hi = min(N, lo + bs)
            m, v = self.predict_f_multisample(X[lo:hi], S, zs=[None if z is None else _data(z)[:, lo:hi] for z in zs])
            lp = self.likelihood.predict_density(m, v, Y[None, lo:hi].expand(m.shape[0], -1, -1)).sum(-1)
            out[lo:hi] = torch.logsumexp(lp, 0) - float(np.log(S))
        return out

    def predict_mixture(self, X, S, Y=None, zs=None, batch_size=None, _moments=True):
        """The Monte Carlo predictive MIXTURE over S draws through the inner layers (drawn as in ``predict_f_multisample``; ``zs``: one
        [S, N, dim] array or None per layer) -> dict of device tensors: ``mean`` [N, Dout] = (1/S) sum_s E_s[y] and ``var`` [N, Dout] =
        (1/S) sum_s (Var_s[y] + E_s[y]^2) - mean^2, with (E_s, Var_s) the likelihood's ``predict_mean_and_var`` at draw s -- for
        ``MultiClass`` the class probabilities averaged over the draws --, and with ``Y`` also ``log_density`` [N] = logsumexp_s sum_d
        predict_density(m_s, v_s, Y) - log S.  Any likelihood.  Per batch of ``batch_size`` points: one precompute, the layer launch without
        a tail (it leaves the final layer's moments, rows n S + s, and nothing else) and ONE ``iwvi_lik_predict_mixture`` launch."""
        X = _data(X)
        S = int(S)
        if S < 1:
            raise ValueError("S must be >= 1, got %d" % S)
        if X.dim() != 2 or X.shape[1] != self._input_dim():
            raise ValueError("X must be [N, %s], got %s" % (self._input_dim(), tuple(X.shape)))
        Dy = self._output_dim()
        if Dy is None:
            raise ValueError("predict_mixture needs a GP layer as the last layer")
        N = X.shape[0]
        if Y is not None:
            Y_given, Y = Y, _data(Y)
            Yd = target_dim(self.likelihood, Dy)
            if Y.dim() != 2 or Y.shape[0] != N or Y.shape[1] != Yd:
                raise ValueError("Y must be [%d, %s], got %s" % (N, Yd, tuple(Y.shape)))
            # (the check reads the targets on the host: from the array as given, and not at all while a graph is being captured)
            if hasattr(self.likelihood, "check_targets") and not (Y.is_cuda and torch.cuda.is_current_stream_capturing()):
                self.likelihood.check_targets(Y_given)
        elif not _moments:
            raise ValueError("nothing asked for: no Y and no moments")
        zs = self._check_predict_noise("predict_mixture", S, N, zs)
        bs = max(1, self._PREDICT_ROWS // S) if batch_size is None else int(batch_size)
        if bs < 1:
            raise ValueError("batch_size must be >= 1")
        dev = X.device
        desc = self.likelihood.lik_desc() if hasattr(self.likelihood, "lik_desc") else None
        if desc is None:                                             # (an object that only quacks like the Gaussian: is_gaussian)
            desc = _abi.LikDesc()
            desc.type = _abi.LIK_GAUSSIAN
            desc.param[0], desc.param0_dev = self.likelihood.desc_variance()
        if _moments and desc.type == _abi.LIK_STUDENT_T and not desc.param[1] > 2.0:
            raise ValueError("predict_mixture: the Student-t variance needs df > 2 (df = %g); predict_log_density gives the density alone" % desc.param[1])
        res = {}
        if _moments:
            Dm = predictive_dim(self.likelihood, Dy)                 # (HeteroskedasticGaussian: one column per TARGET, half the layer's width)
            res["mean"], res["var"] = (torch.empty(N, Dm, dtype=settings.float_type, device=dev) for _ in range(2))
        if Y is not None:
            res["log_density"] = torch.empty(N, dtype=settings.float_type, device=dev)
        if N == 0:
            return res
        self.precompute()
        last = len(self.layers) - 1
        for lo in range(0, N, bs):
            hi = min(N, lo + bs)
            nb = hi - lo
            zb = [None if z is None else _data(z)[:, lo:hi].transpose(0, 1).reshape(nb * S, -1) for z in zs]   # point-major rows n S + s
            _, outs, _ = self._fused_forward(nb * S, S, nb, (nb * S,), zs=zb, sampled_kl=False, want_layers=True, want_logw=False,
                                             use_encoder=False, X=X[lo:hi], outputs_for={last})
            fm, fv = outs[last]["mean"], outs[last]["var"]
            yb = None if Y is None else _abi.dev_tensor(Y[lo:hi].contiguous(), "Y")
            _abi.check(_abi.lib().iwvi_lik_predict_mixture(
                desc, _abi.ptr(fm), _abi.ptr(fv), _abi.ptr(yb), nb, S, Dy, S, 1,
                None if Y is None else _abi.ptr(res["log_density"][lo:hi]),
                _abi.ptr(res["mean"][lo:hi]) if _moments else None, _abi.ptr(res["var"][lo:hi]) if _moments else None, _abi.stream_ptr()))
        return res

    def importance_log_density(self, X, Y, S, proposal="encoder", kind="predictive", zs=None, batch_size=None, return_logw=False):
        """Importance-sampled held-out log density with its diagnostics -> dict of device tensors: ``log_density`` [N] =
        log (1/S) sum_s w_ns, ``log_density_psis`` [N] (the same with the Pareto-smoothed tail), ``khat`` [N] (below 0.5 good, below 0.7
        usable, from 0.7 on unreliable at any practical S; +inf: no fit), ``ess`` [N] (Kish) and, with ``return_logw``, ``logw`` [N, S].

        ``proposal="encoder"``: every latent-variable layer draws w_s ~ q(w | x*, y*) from its encoder on the held-out rows and the draw is
        weighted by p(w_s) / q(w_s | x*, y*): log w = log p(y* | f_s) - sum over those layers of [log q(w_s) - log p(w_s)].
        ``proposal="prior"``: w_s ~ p(w), no weight -- ``predict_log_density``'s estimator plus diagnostics, and the route of a model
        without a latent-variable layer.  Both estimate the same p(y* | x*).  ``kind="predictive"``: p(y* | f_s) is the likelihood's
        predictive density at the final layer's moments; ``kind="bound"``: its variational expectation -- the per-point held-out
        importance-weighted bound without the global KL.  ``zs``: one [S, N, dim] array or None per layer, as ``predict_log_density``.

        Per batch of ``batch_size`` points (default ``_PREDICT_ROWS // S``): one precompute (with the encoders on the batch's [x, y] rows),
        one layer launch (rows n S + s; the final layer's moments and every local regulariser, nothing else), for a likelihood other than
        the Gaussian its elementwise density launch, and one ``iwvi_psis_summary`` launch.  The model's minibatch and its per-minibatch
        caches are as they were afterwards; a call without ``zs`` draws noise, as every predictive call does."""
        from . import psis as _psis
        X, Y = _data(X), _data(Y)
        S = int(S)
        if proposal not in ("encoder", "prior"):
            raise ValueError("proposal is 'encoder' or 'prior', not %r" % (proposal,))
        if kind not in ("predictive", "bound"):
            raise ValueError("kind is 'predictive' or 'bound', not %r" % (kind,))
        if not 1 <= S <= _psis.MAX_S:
            raise ValueError("importance_log_density: S must be in 1..%d (a point's draws are sorted in LDS), got %d" % (_psis.MAX_S, S))
        lv = [i for i, l in enumerate(self.layers) if isinstance(l, LatentVariableLayer)]
        enc = proposal == "encoder" and bool(lv)
        if enc and len(lv) > _abi.MAX_KL:
            raise ValueError("importance_log_density: %d latent-variable layers, the weight takes at most %d local regularisers (IWVI_MAX_KL)"
                             % (len(lv), _abi.MAX_KL))
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("importance_log_density evaluates on one rank only (world size %d): run it outside the sharded group"
                                      % dist.get_world_size())
        if X.dim() != 2 or X.shape[1] != self._input_dim():
            raise ValueError("X must be [N, %s], got %s" % (self._input_dim(), tuple(X.shape)))
        Dy = self._output_dim()
        if Dy is None:
            raise ValueError("importance_log_density needs a GP layer as the last layer")
        Yd = target_dim(self.likelihood, Dy)
        N = X.shape[0]
        if Y.dim() != 2 or Y.shape[0] != N or Y.shape[1] != Yd:
            raise ValueError("Y must be [%d, %s], got %s" % (N, Yd, tuple(Y.shape)))
        zs = self._check_predict_noise("importance_log_density", S, N, zs)
        bs = max(1, self._PREDICT_ROWS // S) if batch_size is None else int(batch_size)
        if bs < 1:
            raise ValueError("batch_size must be >= 1")
        dev = X.device
        names = {"raw": "log_density", "psis": "log_density_psis", "khat": "khat", "ess": "ess"}
        res = {v: torch.empty(N, dtype=settings.float_type, device=dev) for v in names.values()}
        if return_logw:
            res["logw"] = torch.empty(N, S, dtype=settings.float_type, device=dev)
        if N == 0:
            return res
        gauss = is_gaussian(self.likelihood)
        last = len(self.layers) - 1
        # the layer launch takes [x, y] rows and cached encoder outputs from the model's CURRENT minibatch: the held-out batch is bound as
        # that minibatch for the call, with fresh cache buffers (the training ones are not written), and everything is put back
        held = (self.X, self.Y, self._mb_serial, getattr(self, "_xy_cache", None), getattr(self, "_xy_key", None),
                [(getattr(self.layers[i], "_enc_out", None), getattr(self.layers[i], "_enc_key", None)) for i in lv])
        try:
            if not enc:
                self.precompute()
            for lo in range(0, N, bs):
                hi = min(N, lo + bs)
                nb = hi - lo
                xb, yb = _abi.dev_tensor(X[lo:hi].contiguous(), "X"), _abi.dev_tensor(Y[lo:hi].contiguous(), "Y")
                zb = [None if z is None else _data(z)[:, lo:hi].transpose(0, 1).reshape(nb * S, -1) for z in zs]   # point-major rows n S + s
                if enc:
                    self.X, self.Y = xb, yb
                    self._mb_serial += 1
                    self._xy_cache = None
                    for i in lv:
                        self.layers[i]._enc_out = None
                    self.precompute(with_encoders=True)
                _, outs, _ = self._fused_forward(nb * S, S, nb, (nb * S,), zs=zb, sampled_kl=enc, want_layers=True, want_logw=False,
                                                 use_encoder=enc, X=xb, outputs_for={last}, local_kls=enc)
                fm, fv = outs[last]["mean"], outs[last]["var"]
                kls = [outs[i]["kl_local"].reshape(nb * S, -1) for i in lv] if enc else []
                out = {k: res[v][lo:hi] for k, v in names.items()}
                if return_logw:
                    out["logw"] = res["logw"][lo:hi]
                if gauss:
                    lik_host, lik_dev = self.likelihood.desc_variance()
                    _psis.summarise(nb, S, S, 1, fmean=fm, fvar=fv, Y=yb, Dy=Dy, var_exp=kind == "bound", lik_variance=lik_host,
                                    lik_variance_dev=lik_dev, kls=kls, out=out)
                else:
                    terms = torch.empty(nb * S, Yd, dtype=settings.float_type, device=dev)
                    fn = _abi.lib().iwvi_lik_var_exp if kind == "bound" else _abi.lib().iwvi_lik_predict_density
                    _abi.check(fn(self.likelihood.lik_desc(), _abi.ptr(fm), _abi.ptr(fv), _abi.ptr(yb), nb * S, Dy, S, nb, _abi.ptr(terms),
                                  _abi.stream_ptr()))
                    _psis.summarise(nb, S, S, 1, terms=terms, n_terms=Yd, kls=kls, out=out)
        finally:
            self.X, self.Y, self._mb_serial, self._xy_cache, self._xy_key, encs = held
            for i, (eo, ek) in zip(lv, encs):
                self.layers[i]._enc_out, self.layers[i]._enc_key = eo, ek
        return res

    def _check_predict_noise(self, what, S, N, zs):
        """``zs`` of the fused predictive routes: one [S, N, dim] array or None per layer; no fed latent-variable placeholders."""
        zs = [None] * len(self.layers) if zs is None else list(zs)
        if len(zs) != len(self.layers):
            raise ValueError("zs needs one entry per layer")
        for i, (l, z) in enumerate(zip(self.layers, zs)):
            if isinstance(l, LatentVariableLayer) and (l.q_mu_placeholder is not None or l.q_sqrt_placeholder is not None):
                raise ValueError("layer %d: fed latent-variable placeholders are not supported by %s" % (i, what))
            if z is not None:
                w = l.latent_dim if isinstance(l, LatentVariableLayer) else l.num_outputs
                if tuple(z.shape) != (S, N, w):
                    raise ValueError("zs[%d] must be [S, N, %d] = %s, got %s" % (i, w, (S, N, w), tuple(z.shape)))
        return zs

    def predict_y_samples_fused(self, X, S, zs=None, z_y=None, batch_size=None):
        """``predict_y_samples`` [S, N, Dy] in one launch per batch of points: one precompute, then per ``batch_size`` points one
        ``iwvi_dgp_predict_samples`` call (the fused forward with a sampling tail; no per-layer sample, mean or variance reaches memory).
        ``zs``: one [S, N, dim] array or None per layer, ``z_y`` [S, N, Dy] the likelihood's noise -- with both given the result is
        ``predict_y_samples(X, S, zs, z_y)``; what is not given is drawn in the kernel.  The result is a transposed view of the kernel's
        [N, S, Dy], in which a point's S samples are contiguous (what ``evaluation.sample_stats`` reads fastest)."""
        if not is_gaussian(self.likelihood):
            raise NotImplementedError("predict_y_samples_fused adds Gaussian noise in the launch's tail; with %s use predict_y_draws (exact "
                                      "draws of the targets from the likelihood), predict_mixture (the predictive mixture's moments and "
                                      "log density over S draws) or predict_y_samples (layer by layer, the moment-matched m + z sqrt(v) of "
                                      "the likelihood's predict_mean_and_var)" % type(self.likelihood).__name__)
        X = _data(X)
        S = int(S)
        if S < 1:
            raise ValueError("S must be >= 1, got %d" % S)
        if X.dim() != 2 or X.shape[1] != self._input_dim():
            raise ValueError("X must be [N, %s], got %s" % (self._input_dim(), tuple(X.shape)))
        Dy = self._output_dim()
        if Dy is None:
            raise ValueError("predict_y_samples_fused needs a GP layer as the last layer")
        N = X.shape[0]
        zs = self._check_predict_noise("predict_y_samples_fused", S, N, zs)
        if z_y is not None and tuple(z_y.shape) != (S, N, Dy):
            raise ValueError("z_y must be [S, N, %d] = %s, got %s" % (Dy, (S, N, Dy), tuple(z_y.shape)))
        bs = max(1, self._PREDICT_ROWS // S) if batch_size is None else int(batch_size)
        if bs < 1:
            raise ValueError("batch_size must be >= 1")
        out = torch.empty(N, S, Dy, dtype=settings.float_type, device=X.device)
        if N == 0:
            return out.transpose(0, 1)
        self.precompute()
        for lo in range(0, N, bs):
            hi = min(N, lo + bs)
            nb = hi - lo
            zb = [None if z is None else _data(z)[:, lo:hi].transpose(0, 1).reshape(nb * S, -1) for z in zs]   # point-major rows n S + s
            zyb = None if z_y is None else _abi.dev_tensor(_data(z_y)[:, lo:hi].transpose(0, 1).reshape(nb * S, Dy).contiguous(), "z_y")
            self._fused_forward(nb * S, S, nb, (nb * S,), zs=zb, want_logw=False, use_encoder=False,
                                X=X[lo:hi], predict=dict(S=S, out_y=out[lo:hi], z_y=zyb))
        return out.transpose(0, 1)

    def predict_y_draws(self, X, S, zs=None, z_f=None, batch_size=None, return_f=False, serial=None):
        """EXACT draws of the predictive targets [S, N, Dt] for any likelihood: y ~ p(y | f), f ~ N(m_s, v_s) over S draws through the inner
        layers (drawn as in ``predict_f_multisample``; ``zs``: one [S, N, dim] array or None per layer) -- counts for a Poisson, labels for
        a Bernoulli / Ordinal / MultiClass (Dt = 1 there; Dt = Dy / 2 for a HeteroskedasticGaussian; else Dt = Dy), heavy tails for a Student-t --, where ``predict_y_samples`` stays
        the reference's moment-matched ``m + z sqrt(v)``.  Per batch of ``batch_size`` points: one precompute, the layer launch without a
        tail (the final layer's moments, rows n S + s) and ONE ``iwvi_lik_sample_y`` launch on them.  ``z_f`` [S, N, Dy]: the standard
        normals of f (drawn when None); ``return_f``: also the f that was used, [S, N, Dy].  Both results are transposed views of
        [N, S, .] buffers, in which a point's S draws are contiguous (what ``evaluation.sample_stats`` reads fastest).
        The draws' serial lives with the model's device words and every launch advances it: a captured call replays with fresh draws, and
        every batch has a serial of its own -- so the bits depend on ``batch_size``, the distribution does not.  ``serial``: a host
        serial instead (batch i takes ``serial + i``): the same call then gives the same bits."""
        X = _data(X)
        S = int(S)
        if S < 1:
            raise ValueError("S must be >= 1, got %d" % S)
        if X.dim() != 2 or X.shape[1] != self._input_dim():
            raise ValueError("X must be [N, %s], got %s" % (self._input_dim(), tuple(X.shape)))
        Dy = self._output_dim()
        if Dy is None:
            raise ValueError("predict_y_draws needs a GP layer as the last layer")
        N = X.shape[0]
        zs = self._check_predict_noise("predict_y_draws", S, N, zs)
        if z_f is not None and tuple(z_f.shape) != (S, N, Dy):
            raise ValueError("z_f must be [S, N, %d] = %s, got %s" % (Dy, (S, N, Dy), tuple(z_f.shape)))
        bs = max(1, self._PREDICT_ROWS // S) if batch_size is None else int(batch_size)
        if bs < 1:
            raise ValueError("batch_size must be >= 1")
        desc = self.likelihood.lik_desc() if hasattr(self.likelihood, "lik_desc") else None
        if desc is None:                                             # (an object that only quacks like the Gaussian: is_gaussian)
            desc = _abi.LikDesc()
            desc.type = _abi.LIK_GAUSSIAN
            desc.param[0], desc.param0_dev = self.likelihood.desc_variance()
        Dt = target_dim(self.likelihood, Dy)
        dev = X.device
        out = torch.empty(N, S, Dt, dtype=settings.float_type, device=dev)
        out_f = torch.empty(N, S, Dy, dtype=settings.float_type, device=dev) if return_f else None
        if N:
            self.precompute()
        last = len(self.layers) - 1
        for i, lo in enumerate(range(0, N, bs)):
            hi = min(N, lo + bs)
            nb = hi - lo
            zb = [None if z is None else _data(z)[:, lo:hi].transpose(0, 1).reshape(nb * S, -1) for z in zs]   # point-major rows n S + s
            zfb = None if z_f is None else _abi.dev_tensor(_data(z_f)[:, lo:hi].transpose(0, 1).reshape(nb * S, Dy).contiguous(), "z_f")
            _, outs, _ = self._fused_forward(nb * S, S, nb, (nb * S,), zs=zb, sampled_kl=False, want_layers=True, want_logw=False,
                                             use_encoder=False, X=X[lo:hi], outputs_for={last})
            _abi.check(_abi.lib().iwvi_lik_sample_y(
                desc, _abi.ptr(outs[last]["mean"]), _abi.ptr(outs[last]["var"]), nb * S, Dy, _abi.ptr(zfb), settings.seed,
                0 if serial is None else int(serial) + i,
                ctypes.c_void_p(self._words().data_ptr() + 24) if serial is None else None,
                _abi.ptr(out[lo:hi]), None if out_f is None else _abi.ptr(out_f[lo:hi]), _abi.stream_ptr()))
        return (out.transpose(0, 1), out_f.transpose(0, 1)) if return_f else out.transpose(0, 1)

    def predict_y_samples(self, X, S, zs=None, z_y=None):
        X = _data(X)
        X_tiled = X[None, :, :].expand(S, *X.shape).contiguous()       # :104
        _, means, covs, _, _ = self.propagate(X_tiled, zs=zs)
        m, v = self.likelihood.predict_mean_and_var(means[-1], covs[-1])   # :105
        z = draw_normal(m.shape, m.device) if z_y is None else z_y
        return m + z * v ** 0.5                                        # :106-107


class DGP_IWVI(DGP_VI):
    ENCODER_GRADIENTS = ("iwae", "dreg", "stl")
    # ``bound`` (a ``Bound`` or a string for ``Bound.parse``; default ``Bound.iwae()``): with the default every route is the one it was -- the
    # fused tail, the fused heads, K-sharding --; any other member goes precompute, layer launch with its log-weights, ``iwvi_bound_logw_reduce``
    # (``_build_likelihood`` / ``compute_log_likelihood`` / ``E_log_p_Y``, which then returns bound_n), and ``iwvi_bound_elbo_backward`` for the
    # heads of the adjoint (backward.py).  Gaussian likelihood, one rank, the 'iwae' encoder-gradient estimator.
    BOUND_FAMILY = True

    def _joint_over_samples(self):
        """True when some non-final GPLayer has a plain kernel and K > 1: the reference then samples that layer with the
        full [K, K] covariance over the importance samples (models.py:122-125 -> temp_workaround.py:149-155), which the
        fused marginal-sampling launch does not reproduce."""
        return self.num_samples > 1 and any(isinstance(l, GPLayer) and not hasattr(l.kern, "W") for l in self.layers[:-1])

    def _literal(self):
        return self.full_cov_over_samples or self._joint_over_samples()

    def _forward_iw(self, zs=None, _last_sample=True):
        """models.py:113-133 with every per-layer output exposed (tests / API parity).  Default: one fused
        launch, marginal variances everywhere.  With ``full_cov_over_samples`` the reference is followed
        literally (explicit tiling, full_cov=True, matrix_diag_part of the [B, Dy, K, K] covariance)."""
        B, K = self.X.shape[0], self.num_samples
        if self._literal():
            X_tiled = self.X[:, None, :].expand(B, K, self.X.shape[1]).contiguous()     # :113
            Y_tiled = self.Y[:, None, :].expand(B, K, self.Y.shape[1]).contiguous()     # :114
            XY = torch.cat([X_tiled, Y_tiled], -1)                                       # :116
            samples, means, covs, kls, kl_types = self.propagate(
                X_tiled, full_cov=True, inference_amorization_inputs=XY,
                is_sampled_local_regularizer=True, zs=zs, _kl_parts=True, _last_sample=_last_sample)   # :122-125
            local_kls = [kl for kl, t in zip(kls, kl_types) if t is RegularizerType.LOCAL]
            global_kls = [kl for kl, t in zip(kls, kl_types) if t is RegularizerType.GLOBAL]
            cov = covs[-1]
            if cov.dim() == 4:                                                            # [B, Dy, K, K]
                cov = torch.diagonal(cov, dim1=-2, dim2=-1).transpose(1, 2).contiguous()  # :133
            return means[-1], cov, local_kls, global_kls, samples, means, covs
        self.precompute(with_encoders=True)
        _, outs, _ = self._fused_forward(B * K, K, B, (B, K), zs=zs, sampled_kl=True, want_layers=True,
                                         want_logw=is_gaussian(self.likelihood))
        samples, means, covs = ([o[k] for o in outs] for k in ("sample", "mean", "var"))
        local_kls = [o["kl_local"] for o, l in zip(outs, self.layers) if l.regularizer_type is RegularizerType.LOCAL]
        return means[-1], covs[-1], local_kls, self._global_kls(), samples, means, covs

    def _logw(self, zs=None):
        """Per-sample log-weights L_NK [B*K] (models.py:134-142) and the global KL shares."""
        B, K = self.X.shape[0], self.num_samples
        if self._literal():
            return None
        if not is_gaussian(self.likelihood):
            raise NotImplementedError("the per-sample log-weights come out of the Gaussian tail of the layer launch; E_log_p_Y / "
                                      "lse_partials give the reduced forms for %s" % type(self.likelihood).__name__)
        self.precompute(with_encoders=True)
        return self._fused_forward(B * K, K, B, (B, K), zs=zs, sampled_kl=True)[0]

    def _check_bound(self, what=None):
        """What a non-default ``bound`` refuses at the model, before anything is queued (each message names the limit)."""
        bound = self.bound
        bound.check_samples(self.num_samples)
        if what is not None:
            raise NotImplementedError("bound %s: %s" % (bound, what))
        if not is_gaussian(self.likelihood):
            raise NotImplementedError("bound %s: the bound family has the closed-form Gaussian policy only (csrc/bound_family.hip); a %s "
                                      "model has the default bound 'iwae'" % (bound, type(self.likelihood).__name__))
        if self._literal():
            raise NotImplementedError("bound %s: the literal full_cov_over_samples path (and an inner plain-kernel GPLayer, which takes "
                                      "it) reduces with the importance-weighted bound only" % (bound,))

    def _reduce_bound(self, logw, bound, elbo_out=None, want_logp=True, want_ess=False):
        """``iwvi_bound_logw_reduce`` on the layer launch's log-weights [B * K] -> (bound or None, bound_n [B] or None, ess [B] or None)."""
        B, K, dev = self.X.shape[0], self.num_samples, logw.device
        glob = [_abi.dev_tensor(g.reshape(-1), "global kl", torch.float64) for g in self._global_kls()]
        glob_n = (ctypes.c_int32 * max(len(glob), 1))(*[g.numel() for g in glob])
        logp = torch.empty(B, dtype=settings.float_type, device=dev) if want_logp else None
        ess = torch.empty(B, dtype=settings.float_type, device=dev) if want_ess else None
        elbo = None
        if want_logp:
            elbo = torch.empty(1, dtype=torch.float64, device=dev) if elbo_out is None else _abi.dev_tensor(elbo_out.view(-1), "elbo_out", torch.float64)
        _abi.check(_abi.lib().iwvi_bound_logw_reduce(
            bound.desc(), _abi.ptr(logw), B, K, K, 1, _abi.ptr_array(glob), glob_n, len(glob), float(self.num_data) / float(B),
            _abi.ptr(logp), _abi.ptr(ess), _abi.ptr(elbo), _abi.ptr(self._words()), _abi.stream_ptr()))
        return (None if elbo is None else elbo[0]), logp, ess

    def importance_ess(self, zs=None):
        """Kish's effective sample size of every point's K importance weights [B], in [1, K]: (sum_k w_k)^2 / sum_k w_k^2 with
        w_k = exp(L_nk).  Over all K samples, whatever ``bound`` is (the default included).  Two launches and the reduction.
        The ESS looks healthy on a heavy tail until the one huge weight shows up: ``evaluation.psis_summary(model._logw().view(B, K))`` gives
        the same ESS together with the Pareto-k diagnostic, which says whether the weights can be trusted at all."""
        logw = self._logw(zs)
        if logw is None:
            raise NotImplementedError("importance_ess reads the layer launch's log-weights; the literal full_cov_over_samples path has none")
        return self._reduce_bound(logw, Bound(), want_logp=False, want_ess=True)[2]

    def _elbo_parts(self, zs=None, want_ms=False, K_total=None, ms_out=None, elbo_out=None):
        B, K = self.X.shape[0], self.num_samples
        if not self.bound.is_default:
            # precompute, the layer launch with its log-weights, iwvi_bound_logw_reduce: the fused tail holds the log-sum-exp over all K
            self._check_bound()
            if want_ms or ms_out is not None or K_total is not None:
                self._check_bound("lse_partials / K_total exchange the importance-weighted bound's (max, sum exp) pairs: K-sharding has the "
                                  "default bound only")
            el, logp, _ = self._reduce_bound(self._logw(zs), self.bound, elbo_out=elbo_out)
            return el, logp, None
        if self._literal():                                         # literal reference path, layer by layer
            fmean, fvar, local_kls, global_kls, _, _, _ = self._forward_iw(zs, _last_sample=False)
            return self._reduce(fmean, fvar, self.Y, local_kls, global_kls, B, K, stride_b=K, stride_k=1,
                                mode_vi=False, want_ms=want_ms, K_total=K_total,
                                **({} if is_gaussian(self.likelihood) else dict(ms_out=ms_out, elbo_out=elbo_out)))
        if not is_gaussian(self.likelihood):                         # three launches: precompute, layers, iwvi_lik_elbo_reduce
            self.precompute(with_encoders=True)
            return self._moments_then_reduce(B * K, K, B, (B * K,), zs, True,
                                             dict(B=B, K=K, stride_b=K, stride_k=1, mode_vi=False, want_ms=want_ms, K_total=K_total,
                                                  ms_out=ms_out, elbo_out=elbo_out))
        el = dict(B=B, K=K, stride_b=K, stride_k=1, mode_vi=False, want_ms=want_ms, K_total=K_total,
                  ms_out=ms_out, elbo_out=elbo_out)
        if self.lv_in_precompute and isinstance(self.layers[0], LatentVariableLayer) and (zs is None or zs[0] is None):
            # the leading latent-variable layer rides in the precompute launch, beside the factorisations
            self.precompute(with_encoders=True, sample_first=dict(K=K, sampled_kl=True, want_z=self.keep_lv_noise))
            return self._fused_forward(B * K, K, B, (B, K), zs=None if zs is None else zs[1:], sampled_kl=True,
                                       elbo=el, stack_from=1)[2]
        self.precompute(with_encoders=True)
        return self._fused_forward(B * K, K, B, (B, K), zs=zs, sampled_kl=True, elbo=el)[2]

    def _build_likelihood(self, zs=None, out=None):
        """The importance-weighted ELBO, reference models.py:112-150 (``out``: optional 1-element float64 result buffer)."""
        return self._elbo_parts(zs, elbo_out=out)[0]

    def E_log_p_Y(self, zs=None):
        """Per-point ``logsumexp_k(L_nk) - log K`` [B] (models.py:134-148); name from BASELINE.json."""
        return self._elbo_parts(zs)[1]

    def lse_partials(self, zs=None, K_total=None, out=None):
        """(max_k L, sum_k exp(L - max)) per point [B, 2] + the global KLs: the K-sharded exchange unit
        (``out``: optional [B, 2] buffer to write the pairs into)."""
        _, _, ms = self._elbo_parts(zs, want_ms=True, K_total=K_total, ms_out=out)
        return ms, self._global_kls()
