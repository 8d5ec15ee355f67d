"""Likelihoods (GPflow-1.x ``gpflow.likelihoods`` counterparts; reference: experiments/build_models.py:198-199; models.py:66,105,134).

``Gaussian``: on the hot path ``variational_expectations`` is fused into the tail of ``iwvi_dgp_forward``; the method here is the
reference's callable form on explicit moments (``iwvi_gaussian_var_exp``); ``logp`` / ``predict_density`` run
``iwvi_gaussian_log_density``.

``Bernoulli`` (probit link) and ``StudentT`` are the non-conjugate ones: their expectations are GPflow's 20-point Gauss-Hermite rule,
evaluated by the kernels of ``csrc/likelihood_tail.hip`` (``iwvi_lik_*``).  A model with one of them runs the layer launch without its
Gaussian tail and ``iwvi_lik_elbo_reduce`` / ``iwvi_lik_elbo_backward`` on the final layer's moments (models.py, backward.py).

Every likelihood answers ``lik_desc()`` (the ``iwvi_lik_desc`` of its current parameters), ``grad_name`` (the key of its trained scalar's
gradient in ``backward.iw_elbo_and_gradients``, or None) and ``trained_scalar()`` (what a ``training.Trainer`` puts among its Adam
scalars: (gradient name, value), or None).

``MultiClass`` (robust-max link; ``csrc/likelihood_multiclass.hip``) is the one likelihood whose targets are not as wide as the final
layer: ``Y`` is ONE column of class labels 0 .. C-1 while the layer has C outputs.  Nothing equates the two widths directly: ``target_dim``
/ ``output_dim`` below translate, and a likelihood says which it is by a ``num_classes`` attribute.

``HeteroskedasticGaussian`` (``csrc/likelihood_hetero.hip``) is the other one: TWO outputs of the final layer per target column, the mean
and the log noise variance (``outputs_per_target = 2``).  Closed-form expectations like the exp-link three; nothing is trained.

``Poisson``, ``Exponential`` and ``Gamma`` (exp link, GPflow's default; ``csrc/likelihood_explink.hip``) have closed-form variational
expectations -- one ``exp`` per element, no quadrature --; ``Gamma.shape`` is the one trained scalar (``grad_name`` 'lik_shape').

``Beta`` (targets in [0, 1]) and ``Ordinal`` (ordered grades 0 .. n) squash the latent through the probit link; everything is the 20-point
rule again (``csrc/likelihood_bounded.hip``).  ``Beta.scale`` ('lik_scale') and ``Ordinal.sigma`` ('lik_sigma') are trained.  The Ordinal
keeps ONE device buffer [sigma, e_0 .. e_(n-1)] that every launch reads, and hands whoever trains sigma the 1-element view of its head
(``trained_scalar_view``) instead of being bound to a tensor of the trainer's."""
import math

import torch

from . import _abi, settings
from .kernels import DeviceScalarVariance


def target_dim(likelihood, Dy):
    """Columns of Y for a final layer of ``Dy`` outputs: 1 for a likelihood over class labels (``num_classes``), ``Dy / outputs_per_target``
    for one with several latent functions per target column (``HeteroskedasticGaussian``: 2), else ``Dy``."""
    if getattr(likelihood, "num_classes", None) is not None:
        return 1
    per = getattr(likelihood, "outputs_per_target", 1)
    return Dy if per == 1 or Dy is None else Dy // per


def output_dim(likelihood, y_dim):
    """The other way round: outputs of the final layer (columns of its moments and of the heads) for targets of ``y_dim`` columns."""
    C = getattr(likelihood, "num_classes", None)
    return y_dim * getattr(likelihood, "outputs_per_target", 1) if C is None else C


def predictive_dim(likelihood, Dy):
    """Columns of ``predict_mean_and_var`` (and of a predictive mixture's mean / var) for a final layer of ``Dy`` outputs: one per class
    for ``MultiClass``, otherwise one per target column."""
    return Dy if getattr(likelihood, "num_classes", None) is not None else target_dim(likelihood, Dy)


def desc_target_dim(desc, Dy):
    """``target_dim`` from a descriptor alone (``sample_y_launch``)."""
    return 1 if desc.type == _abi.LIK_MULTICLASS else Dy // 2 if desc.type == _abi.LIK_HETERO_GAUSSIAN else Dy


def _moments(Fmu, Fvar, Y, likelihood=None):
    """(Fmu, Fvar or None, Y or None, T, Dy) as contiguous device tensors of Fmu's shape (Y: ``target_dim`` columns)."""
    Fmu = _abi.dev_tensor(torch.as_tensor(Fmu).contiguous(), "Fmu")
    if Fvar is not None:
        Fvar = _abi.dev_tensor(torch.as_tensor(Fvar, device=Fmu.device).expand_as(Fmu).contiguous(), "Fvar")
    Dy = Fmu.shape[-1] if Fmu.dim() else 1
    if Y is not None:
        y_shape = tuple(Fmu.shape[:-1]) + (target_dim(likelihood, Dy),) if Fmu.dim() else ()
        Y = _abi.dev_tensor(torch.as_tensor(Y, dtype=settings.float_type, device=Fmu.device).expand(y_shape).contiguous(), "Y")
    return Fmu, Fvar, Y, Fmu.numel() // max(Dy, 1), Dy


def sample_y_launch(desc, Fmu, Fvar, z_f=None, return_f=False, seed=None, serial=None):
    """One ``iwvi_lik_sample_y`` launch on contiguous device moments [..., Dy] for the descriptor ``desc`` -> y [..., Dt] (Dt = 1 for the
    MultiClass, Dy / 2 for the heteroskedastic Gaussian, else Dy), or (y, f) with ``return_f``."""
    Fmu, Fvar, _, T, Dy = _moments(Fmu, Fvar, None)
    if z_f is not None:
        z_f = _abi.dev_tensor(torch.as_tensor(z_f, device=Fmu.device).expand_as(Fmu).contiguous(), "z_f")
    Dt = desc_target_dim(desc, Dy)
    out_y = torch.empty(*Fmu.shape[:-1], Dt, dtype=Fmu.dtype, device=Fmu.device) if Fmu.dim() else torch.empty_like(Fmu)
    out_f = torch.empty_like(Fmu) if return_f else None
    if Fmu.numel() == 0:                                             # (an empty tensor has no address to hand over: nothing to launch)
        return (out_y, out_f) if return_f else out_y
    _abi.check(_abi.lib().iwvi_lik_sample_y(desc, _abi.ptr(Fmu), _abi.ptr(Fvar), T, Dy, _abi.ptr(z_f),
                                            settings.seed if seed is None else int(seed),
                                            settings.next_sample_serial() if serial is None else int(serial),
                                            None, _abi.ptr(out_y), _abi.ptr(out_f), _abi.stream_ptr()))
    return (out_y, out_f) if return_f else out_y


class _SampleY:
    """``sample_y`` of every likelihood: exact draws of a target, one ``iwvi_lik_sample_y`` launch (``csrc/likelihood_sample.hip``)."""

    def sample_y(self, Fmu, Fvar, z_f=None, return_f=False, seed=None, serial=None):
        """y ~ p(y | f), f = Fmu + sqrt(Fvar) z (``Fvar`` None: f = Fmu), elementwise on device moments [..., Dy] -> [..., Dy] (MultiClass:
        [..., 1] labels; HeteroskedasticGaussian: [..., Dy / 2], with ``z_f`` / ``return_f`` [..., Dy] covering the mean and the log noise
        variance).  ``z_f``: the standard normals of f, drawn when None; ``return_f``: also the f that was used.  The noise is the
        sub-stream (``seed``, ``serial``) per element: ``settings.seed`` and the next serial of ``settings.next_sample_serial`` by default,
        the same pair gives the same bits."""
        return sample_y_launch(self.lik_desc(), Fmu, Fvar, z_f=z_f, return_f=return_f, seed=seed, serial=serial)


class _QuadratureLikelihood(_SampleY):
    """The methods of a likelihood whose arithmetic lives in ``csrc/likelihood_tail.hip``."""

    def variational_expectations(self, Fmu, Fvar, Y):
        """E_{N(f; Fmu, Fvar)} logp(f, Y), elementwise, by the 20-point Gauss-Hermite rule (GPflow 1.x ``ndiagquad``; models.py:66,134)."""
        Fmu, Fvar, Y, T, Dy = _moments(Fmu, Fvar, Y)
        out = torch.empty_like(Fmu)
        d = self.lik_desc()
        _abi.check(_abi.lib().iwvi_lik_var_exp(d, _abi.ptr(Fmu), _abi.ptr(Fvar), _abi.ptr(Y), T, Dy, 1, max(T, 1), _abi.ptr(out), _abi.stream_ptr()))
        return out

    def _density(self, Fmu, Fvar, Y):
        Fmu, Fvar, Y, T, Dy = _moments(Fmu, Fvar, Y)
        out = torch.empty_like(Fmu)
        d = self.lik_desc()
        _abi.check(_abi.lib().iwvi_lik_predict_density(d, _abi.ptr(Fmu), _abi.ptr(Fvar), _abi.ptr(Y), T, Dy, 1, max(T, 1), _abi.ptr(out),
                                                       _abi.stream_ptr()))
        return out

    def logp(self, F, Y):
        return self._density(F, None, Y)

    def predict_density(self, Fmu, Fvar, Y):
        return self._density(Fmu, Fvar, Y)

    def predict_mean_and_var(self, Fmu, Fvar):
        Fmu, Fvar, _, _, _ = _moments(Fmu, Fvar, None)
        m, v = torch.empty_like(Fmu), torch.empty_like(Fmu)
        d = self.lik_desc()
        _abi.check(_abi.lib().iwvi_lik_predict_mean_and_var(d, _abi.ptr(Fmu), _abi.ptr(Fvar), Fmu.numel(), _abi.ptr(m), _abi.ptr(v),
                                                            _abi.stream_ptr()))
        return m, v


class Gaussian(_SampleY, DeviceScalarVariance):
    def __init__(self, variance=1.0, name=None):
        self.variance = float(variance)
        self.name = name

    def lik_desc(self):
        d = _abi.LikDesc()
        d.type = _abi.LIK_GAUSSIAN
        d.param[0], d.param0_dev = self.desc_variance()
        return d

    grad_name = "lik_var"

    def trained_scalar(self):
        return self.grad_name, self.variance

    def variational_expectations(self, Fmu, Fvar, Y):
        """E_{N(f; Fmu, Fvar)} log N(Y; f, variance), elementwise (gpflow 1.x Gaussian; called at models.py:66,134)."""
        Fmu = _abi.dev_tensor(Fmu.contiguous(), "Fmu")
        Fvar = _abi.dev_tensor(Fvar.expand_as(Fmu).contiguous(), "Fvar")
        Y = _abi.dev_tensor(torch.as_tensor(Y, dtype=settings.float_type, device=Fmu.device).expand_as(Fmu).contiguous(), "Y")
        out = torch.empty_like(Fmu)
        Dy = Fmu.shape[-1] if Fmu.dim() else 1
        T = Fmu.numel() // max(Dy, 1)
        _abi.check(_abi.lib().iwvi_gaussian_var_exp(_abi.ptr(Fmu), _abi.ptr(Fvar), _abi.ptr(Y), self.variance,
                                                    T, Dy, 1, max(T, 1), _abi.ptr(out), _abi.stream_ptr()))
        return out

    def predict_mean_and_var(self, Fmu, Fvar):
        return Fmu, Fvar + self.variance

    def _log_density(self, Fmu, Fvar, Y):
        Fmu = _abi.dev_tensor(torch.as_tensor(Fmu).contiguous(), "F")
        Fvar = None if Fvar is None else _abi.dev_tensor(torch.as_tensor(Fvar, device=Fmu.device).expand_as(Fmu).contiguous(), "Fvar")
        Y = _abi.dev_tensor(torch.as_tensor(Y, dtype=settings.float_type, device=Fmu.device).expand_as(Fmu).contiguous(), "Y")
        out = torch.empty_like(Fmu)
        Dy = Fmu.shape[-1] if Fmu.dim() else 1
        T = Fmu.numel() // max(Dy, 1)
        host, dev = self.desc_variance()
        _abi.check(_abi.lib().iwvi_gaussian_log_density(_abi.ptr(Fmu), _abi.ptr(Fvar), _abi.ptr(Y), host, dev,
                                                        T, Dy, 1, max(T, 1), _abi.ptr(out), _abi.stream_ptr()))
        return out

    def logp(self, F, Y):
        """log N(Y; F, variance), elementwise (gpflow 1.x Gaussian.logp)."""
        return self._log_density(F, None, Y)

    def predict_density(self, Fmu, Fvar, Y):
        """log N(Y; Fmu, Fvar + variance), elementwise (gpflow 1.x Gaussian.predict_density)."""
        return self._log_density(Fmu, Fvar, Y)


class Bernoulli(_QuadratureLikelihood):
    """gpflow 1.x ``Bernoulli(invlink=inv_probit)``: p = Phi(F) (1 - 2e-3) + 1e-3, logp = log p if Y == 1 else log(1 - p).
    ``predict_mean_and_var`` and ``predict_density`` are the probit link's closed forms at p = inv_probit(Fmu / sqrt(1 + Fvar))."""

    def __init__(self, invlink=None, name=None):
        if invlink is not None and getattr(invlink, "__name__", invlink) != "inv_probit":
            raise NotImplementedError("Bernoulli(invlink=%r): only the probit link (GPflow's default, inv_probit) is implemented"
                                      % (getattr(invlink, "__name__", invlink),))
        self.name = name

    def lik_desc(self):
        d = _abi.LikDesc()
        d.type = _abi.LIK_BERNOULLI_PROBIT
        return d

    grad_name = None

    def trained_scalar(self):
        return None

    def check_targets(self, Y):
        """Labels must be exactly 0 or 1: ``logp`` takes ``Y == 1`` for class 1 and EVERYTHING else (0.999, -1, 2) for class 0, as GPflow
        does, silently.  The models call this once on the host when they are built."""
        import numpy as np
        Yh = Y.detach().cpu().numpy() if isinstance(Y, torch.Tensor) else np.asarray(Y)
        bad = ~((Yh == 0) | (Yh == 1))
        if bad.any():
            raise ValueError("Bernoulli: targets must be 0 or 1; %d of %d are not (first: %r)" % (int(bad.sum()), Yh.size, Yh[bad].ravel()[0]))


def inv_probit(x):
    """GPflow's probit link with its jitter, on torch tensors (the name ``Bernoulli(invlink=...)`` accepts)."""
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) * (1 - 2e-3) + 1e-3


class StudentT(_QuadratureLikelihood, DeviceScalarVariance):
    """gpflow 1.x ``StudentT(scale=1.0, df=3.0)``: ``scale`` is trainable (positive), ``df`` is fixed.  Everything but ``logp`` is
    quadrature; ``predict_mean_and_var`` needs df > 2."""
    # GPflow's name for the one trained scalar: the lazily refreshed host copy / device master of DeviceScalarVariance
    scale = property(DeviceScalarVariance.host_value, DeviceScalarVariance.variance.fset)

    def __init__(self, scale=1.0, df=3.0, name=None):
        if not float(scale) > 0.0:
            raise ValueError("StudentT: scale must be positive, got %r" % (scale,))
        if not float(df) > 0.0:
            raise ValueError("StudentT: df must be positive, got %r" % (df,))
        self.scale = float(scale)
        self.df = float(df)
        self.name = name

    @property
    def variance(self):
        raise AttributeError("StudentT has no 'variance': its parameters are 'scale' and 'df'")

    def lik_desc(self):
        d = _abi.LikDesc()
        d.type = _abi.LIK_STUDENT_T
        d.param[0], d.param0_dev = self.desc_variance()
        d.param[1] = self.df
        d.lgc = math.lgamma(0.5 * (self.df + 1.0)) - math.lgamma(0.5 * self.df)
        return d

    grad_name = "lik_scale"

    def trained_scalar(self):
        return self.grad_name, self.scale

    def predict_mean_and_var(self, Fmu, Fvar):
        if not self.df > 2.0:
            raise ValueError("StudentT.predict_mean_and_var: the variance needs df > 2 (df = %g)" % self.df)
        return super().predict_mean_and_var(Fmu, Fvar)


class RobustMax:
    """gpflow 1.x ``RobustMax(num_classes, epsilon=1e-3)``: the link of ``MultiClass`` -- 1 - epsilon on the largest latent, epsilon / (C - 1)
    on each other."""

    def __init__(self, num_classes, epsilon=1e-3):
        if int(num_classes) != num_classes or not 2 <= int(num_classes) <= _abi.MAX_P:
            raise ValueError("RobustMax: num_classes must be an integer in 2..%d, got %r" % (_abi.MAX_P, num_classes))
        if not 0.0 < float(epsilon) < 1.0:
            raise ValueError("RobustMax: epsilon must lie in (0, 1), got %r" % (epsilon,))
        self.num_classes = int(num_classes)
        self.epsilon = float(epsilon)


class MultiClass(_SampleY):
    """gpflow 1.x ``MultiClass(num_classes)`` with the ``RobustMax`` link (its default).  ``Y`` is ONE column of class labels 0 .. C-1; ``F``,
    ``Fmu`` and ``Fvar`` have C columns.  With p = prob_is_largest(Y; Fmu, Fvar) by the 20-point rule over the label's own latent
    (``csrc/likelihood_multiclass.hip``; clips and the 1e-4 cdf jitter as GPflow's) and eps_1 = epsilon / (C - 1):
    ``variational_expectations`` = p log(1 - epsilon) + (1 - p) log eps_1 and ``predict_density`` = log(p (1 - epsilon) + (1 - p) eps_1), both
    [..., 1]; ``logp`` = log(1 - epsilon) where argmax F == Y (the first maximum wins) else log eps_1, [..., 1]; ``predict_mean_and_var`` =
    (P, P - P^2) [..., C], P_k the predictive probability of class k.  Nothing is trained."""

    def __init__(self, num_classes, invlink=None, name=None):
        if invlink is None:
            invlink = RobustMax(num_classes)
        if not isinstance(invlink, RobustMax):
            shown = invlink if isinstance(invlink, str) else getattr(invlink, "__name__", type(invlink).__name__)
            raise NotImplementedError("MultiClass(invlink=%r): only the robust-max link (GPflow's default, RobustMax) is implemented" % (shown,))
        if invlink.num_classes != num_classes:
            raise ValueError("MultiClass(%r) with a RobustMax over %d classes" % (num_classes, invlink.num_classes))
        self.num_classes = invlink.num_classes
        self.invlink = invlink
        self.name = name

    epsilon = property(lambda self: self.invlink.epsilon)

    def lik_desc(self):
        d = _abi.LikDesc()
        d.type = _abi.LIK_MULTICLASS
        d.param[0], d.param[1] = self.invlink.epsilon, float(self.num_classes)
        return d

    grad_name = None

    def trained_scalar(self):
        return None

    def check_targets(self, Y):
        """Y must be [N, 1] with integral values in [0, C): the kernels index the final layer's outputs with it.  The models call this once
        on the host when they are built."""
        import numpy as np
        Yh = Y.detach().cpu().numpy() if isinstance(Y, torch.Tensor) else np.asarray(Y)
        if Yh.ndim != 2 or Yh.shape[1] != 1:
            raise ValueError("MultiClass: targets must be one column of class labels [N, 1], got shape %s" % (tuple(Yh.shape),))
        bad = ~((Yh >= 0) & (Yh < self.num_classes) & (Yh == np.floor(Yh)))
        if bad.any():
            raise ValueError("MultiClass: targets must be integers in [0, %d); %d of %d are not (first: %r)"
                             % (self.num_classes, int(bad.sum()), Yh.size, Yh[bad].ravel()[0]))

    def check_output_dim(self, Dy):
        """The final layer must have one output per class (the models call this when they are built)."""
        if Dy != self.num_classes:
            raise ValueError("MultiClass(%d) needs a final layer with %d outputs, got %s" % (self.num_classes, self.num_classes, Dy))

    def _rows(self, entry, Fmu, Fvar, Y):
        Fmu, Fvar, Y, T, C = _moments(Fmu, Fvar, Y, self)
        if C != self.num_classes:
            raise ValueError("MultiClass(%d): the moments need %d columns, got %d" % (self.num_classes, self.num_classes, C))
        out = torch.empty(*Fmu.shape[:-1], 1, dtype=Fmu.dtype, device=Fmu.device)
        _abi.check(getattr(_abi.lib(), entry)(self.lik_desc(), _abi.ptr(Fmu), _abi.ptr(Fvar), _abi.ptr(Y), T, C, 1, max(T, 1), _abi.ptr(out),
                                              _abi.stream_ptr()))
        return out

    def variational_expectations(self, Fmu, Fvar, Y):
        return self._rows("iwvi_lik_var_exp", Fmu, Fvar, Y)

    def logp(self, F, Y):
        return self._rows("iwvi_lik_predict_density", F, None, Y)

    def predict_density(self, Fmu, Fvar, Y):
        return self._rows("iwvi_lik_predict_density", Fmu, Fvar, Y)

    def predict_mean_and_var(self, Fmu, Fvar):
        Fmu, Fvar, _, _, C = _moments(Fmu, Fvar, None)
        if C != self.num_classes:
            raise ValueError("MultiClass(%d): the moments need %d columns, got %d" % (self.num_classes, self.num_classes, C))
        m, v = torch.empty_like(Fmu), torch.empty_like(Fmu)
        _abi.check(_abi.lib().iwvi_lik_predict_mean_and_var(self.lik_desc(), _abi.ptr(Fmu), _abi.ptr(Fvar), Fmu.numel(), _abi.ptr(m), _abi.ptr(v),
                                                            _abi.stream_ptr()))
        return m, v


class HeteroskedasticGaussian(_SampleY):
    """A Gaussian whose noise variance is a second latent function of the input (GPflow 2's ``HeteroskedasticTFPConditional`` with the exp
    link; ``csrc/likelihood_hetero.hip``).  For Dt target columns the final layer has 2 Dt outputs: columns 0 .. Dt-1 are the mean function
    f, columns Dt .. 2 Dt-1 are g, the LOG NOISE VARIANCE of the same target column; ``Y`` and every result below are [..., Dt] against
    moments [..., 2 Dt].  ``logp`` = -1/2 log 2 pi - g / 2 - (Y - f)^2 exp(-g) / 2; ``variational_expectations`` is the closed form
    -1/2 log 2 pi - m_g / 2 - ((Y - m_f)^2 + v_f) exp(-m_g + v_g / 2) / 2; ``predict_mean_and_var`` = (m_f, v_f + exp(m_g + v_g / 2));
    ``predict_density`` integrates N(Y; m_f, v_f + exp(g)) over g by the 20-point rule, in log space.  Every exponent is clipped to
    [-60, 60].  No parameter, nothing is trained."""
    outputs_per_target = 2

    def __init__(self, name=None):
        self.name = name

    def lik_desc(self):
        d = _abi.LikDesc()
        d.type = _abi.LIK_HETERO_GAUSSIAN
        return d

    grad_name = None

    def trained_scalar(self):
        return None

    def check_targets(self, Y):
        """Any finite real (the models call this once on the host when they are built)."""
        import numpy as np
        Yh = _host_targets(Y)
        _refuse_targets("HeteroskedasticGaussian", "finite", Yh, ~np.isfinite(Yh))

    def check_output_dim(self, Dy):
        """The final layer must have two outputs per target column (the models call this when they are built)."""
        if Dy is None or int(Dy) != Dy or Dy < 2 or Dy % 2 or Dy > _abi.MAX_P:
            raise ValueError("HeteroskedasticGaussian needs a final layer with an even number of outputs in 2..%d (the means, then the log "
                             "noise variances), got %s" % (_abi.MAX_P, Dy))

    def _rows(self, entry, Fmu, Fvar, Y):
        Fmu, Fvar, Y, T, Dy = _moments(Fmu, Fvar, Y, self)
        self.check_output_dim(Dy)
        out = torch.empty(*Fmu.shape[:-1], Dy // 2, dtype=Fmu.dtype, device=Fmu.device)
        if Fmu.numel() == 0:
            return out
        _abi.check(getattr(_abi.lib(), entry)(self.lik_desc(), _abi.ptr(Fmu), _abi.ptr(Fvar), _abi.ptr(Y), T, Dy, 1, max(T, 1), _abi.ptr(out),
                                              _abi.stream_ptr()))
        return out

    def variational_expectations(self, Fmu, Fvar, Y):
        return self._rows("iwvi_lik_var_exp", Fmu, Fvar, Y)

    def logp(self, F, Y):
        return self._rows("iwvi_lik_predict_density", F, None, Y)

    def predict_density(self, Fmu, Fvar, Y):
        return self._rows("iwvi_lik_predict_density", Fmu, Fvar, Y)

    def predict_mean_and_var(self, Fmu, Fvar):
        Fmu, Fvar, _, _, Dy = _moments(Fmu, Fvar, None)
        self.check_output_dim(Dy)
        m, v = (torch.empty(*Fmu.shape[:-1], Dy // 2, dtype=Fmu.dtype, device=Fmu.device) for _ in range(2))
        if Fmu.numel() == 0:
            return m, v
        d = self.lik_desc()
        d.param[1] = float(Dy)                                    # (the one entry without a Dy argument reads the row width here)
        _abi.check(_abi.lib().iwvi_lik_predict_mean_and_var(d, _abi.ptr(Fmu), _abi.ptr(Fvar), Fmu.numel(), _abi.ptr(m), _abi.ptr(v),
                                                            _abi.stream_ptr()))
        return m, v


def _exp_link_only(cls_name, invlink):
    if invlink is not None and getattr(invlink, "__name__", invlink) != "exp":
        raise NotImplementedError("%s(invlink=%r): only the exp link (GPflow's default) is implemented"
                                  % (cls_name, getattr(invlink, "__name__", invlink)))


def _host_targets(Y):
    import numpy as np
    return Y.detach().cpu().numpy() if isinstance(Y, torch.Tensor) else np.asarray(Y)


def _refuse_targets(cls_name, what, Yh, bad):
    if bad.any():
        raise ValueError("%s: targets must be %s; %d of %d are not (first: %r)" % (cls_name, what, int(bad.sum()), Yh.size, Yh[bad].ravel()[0]))


class Poisson(_QuadratureLikelihood):
    """gpflow 1.x ``Poisson(invlink=exp, binsize=1.0)``: Y ~ Poisson(binsize exp(F)), logp = Y log(binsize exp(F)) - binsize exp(F) -
    lgamma(Y + 1).  ``variational_expectations`` is the closed form Y mu - binsize exp(mu + v / 2) - lgamma(Y + 1) + Y log binsize;
    ``predict_density`` / ``predict_mean_and_var`` are GPflow's defaults by the 20-point rule.  ``binsize`` is fixed; nothing is trained."""

    def __init__(self, invlink=None, binsize=1.0, name=None):
        _exp_link_only("Poisson", invlink)
        if not float(binsize) > 0.0:
            raise ValueError("Poisson: binsize must be positive, got %r" % (binsize,))
        self.binsize = float(binsize)
        self.name = name

    def lik_desc(self):
        d = _abi.LikDesc()
        d.type = _abi.LIK_POISSON
        d.param[0] = self.binsize
        return d

    grad_name = None

    def trained_scalar(self):
        return None

    def check_targets(self, Y):
        """Counts: finite integers >= 0 (the models call this once on the host when they are built)."""
        import numpy as np
        Yh = _host_targets(Y)
        _refuse_targets("Poisson", "finite integers >= 0", Yh, ~(np.isfinite(Yh) & (Yh >= 0) & (Yh == np.floor(Yh))))


class Exponential(_QuadratureLikelihood):
    """gpflow 1.x ``Exponential(invlink=exp)``: Y ~ Exponential with scale exp(F), logp = -Y exp(-F) - F.  ``variational_expectations`` is the
    closed form -Y exp(-mu + v / 2) - mu; ``predict_density`` / ``predict_mean_and_var`` are GPflow's defaults by the 20-point rule.
    No parameter."""

    def __init__(self, invlink=None, name=None):
        _exp_link_only("Exponential", invlink)
        self.name = name

    def lik_desc(self):
        d = _abi.LikDesc()
        d.type = _abi.LIK_EXPONENTIAL
        return d

    grad_name = None

    def trained_scalar(self):
        return None

    def check_targets(self, Y):
        """Finite and >= 0 (the models call this once on the host when they are built)."""
        import numpy as np
        Yh = _host_targets(Y)
        _refuse_targets("Exponential", "finite and >= 0", Yh, ~(np.isfinite(Yh) & (Yh >= 0)))


class Gamma(_QuadratureLikelihood, DeviceScalarVariance):
    """gpflow 1.x ``Gamma(invlink=exp, shape=1.0)``: Y ~ Gamma(shape, scale exp(F)), logp = -shape F - lgamma(shape) + (shape - 1) log Y -
    Y exp(-F).  ``variational_expectations`` is the closed form with exp(-mu + v / 2) in place of exp(-F); ``predict_density`` /
    ``predict_mean_and_var`` are GPflow's defaults by the 20-point rule.  ``shape`` is trainable (positive): lgamma and digamma of it are
    evaluated on the device from the value a launch reads."""
    # the one trained scalar: the lazily refreshed host copy / device master of DeviceScalarVariance, as StudentT.scale
    shape = property(DeviceScalarVariance.host_value, DeviceScalarVariance.variance.fset)

    def __init__(self, invlink=None, shape=1.0, name=None):
        _exp_link_only("Gamma", invlink)
        if not float(shape) > 0.0:
            raise ValueError("Gamma: shape must be positive, got %r" % (shape,))
        self.shape = float(shape)
        self.name = name

    @property
    def variance(self):
        raise AttributeError("Gamma has no 'variance': its parameter is 'shape'")

    def lik_desc(self):
        d = _abi.LikDesc()
        d.type = _abi.LIK_GAMMA
        d.param[0], d.param0_dev = self.desc_variance()
        return d

    grad_name = "lik_shape"

    def trained_scalar(self):
        return self.grad_name, self.shape

    def check_targets(self, Y):
        """Finite and > 0: log Y enters the density (the models call this once on the host when they are built)."""
        import numpy as np
        Yh = _host_targets(Y)
        _refuse_targets("Gamma", "finite and > 0", Yh, ~(np.isfinite(Yh) & (Yh > 0)))


def _probit_link_only(cls_name, invlink):
    if invlink is not None and getattr(invlink, "__name__", invlink) != "inv_probit":
        raise NotImplementedError("%s(invlink=%r): only the probit link (GPflow's default, inv_probit) is implemented"
                                  % (cls_name, getattr(invlink, "__name__", invlink)))


class Beta(_QuadratureLikelihood, DeviceScalarVariance):
    """gpflow 1.x ``Beta(invlink=inv_probit, scale=1.0)``: Y ~ Beta(alpha, beta) with mean m = inv_probit(F), alpha = m scale, beta = scale -
    alpha; logp = (alpha - 1) log Yc + (beta - 1) log(1 - Yc) + lgamma(scale) - lgamma(alpha) - lgamma(beta), Yc = clip(Y, 1e-6, 1 - 1e-6).
    Everything but ``logp`` is GPflow's default by the 20-point rule.  ``scale`` is trainable (positive): lgamma and digamma of it are
    evaluated on the device from the value a launch reads."""
    # the one trained scalar: the lazily refreshed host copy / device master of DeviceScalarVariance, as StudentT.scale
    scale = property(DeviceScalarVariance.host_value, DeviceScalarVariance.variance.fset)

    def __init__(self, invlink=None, scale=1.0, name=None):
        _probit_link_only("Beta", invlink)
        if not float(scale) > 0.0:
            raise ValueError("Beta: scale must be positive, got %r" % (scale,))
        self.scale = float(scale)
        self.name = name

    @property
    def variance(self):
        raise AttributeError("Beta has no 'variance': its parameter is 'scale'")

    def lik_desc(self):
        d = _abi.LikDesc()
        d.type = _abi.LIK_BETA
        d.param[0], d.param0_dev = self.desc_variance()
        return d

    grad_name = "lik_scale"

    def trained_scalar(self):
        return self.grad_name, self.scale

    def check_targets(self, Y):
        """Finite and in [0, 1] (0 and 1 themselves are clipped to 1e-6 and 1 - 1e-6 inside the density, as GPflow does); the models call
        this once on the host when they are built."""
        import numpy as np
        Yh = _host_targets(Y)
        _refuse_targets("Beta", "finite and in [0, 1]", Yh, ~(np.isfinite(Yh) & (Yh >= 0) & (Yh <= 1)))


class Ordinal(_QuadratureLikelihood):
    """gpflow 1.x ``Ordinal(bin_edges)``: n strictly increasing edges make n + 1 bins, Y holds the bin 0 .. n.  With l = e_Y / sigma (+inf
    for the top bin) and r = e_(Y-1) / sigma (-inf for the bottom one), P_Y(F) = inv_probit(l - F / sigma) - inv_probit(r - F / sigma) and
    logp = log(P_Y + 1e-6); the bins sum to 0.998, as GPflow's do.  Everything but ``logp`` is GPflow's default by the 20-point rule.
    ``sigma`` (1.0 at first) is trainable (positive); the edges are fixed.  Both live in ONE device buffer [sigma, e_0 .. e_(n-1)], created
    on the current device at the first use and moved by ``to`` (``model.to`` calls it)."""

    def __init__(self, bin_edges, name=None):
        self.bin_edges = self._checked_edges(bin_edges)
        self._sigma_host, self._stale, self._buf = 1.0, False, None
        self.name = name

    @staticmethod
    def _checked_edges(bin_edges):
        import numpy as np
        edges = np.array(_host_targets(bin_edges), dtype=np.float64).reshape(-1)
        if not 1 <= edges.size <= _abi.MAX_P - 1:
            raise ValueError("Ordinal: 1 to %d bin edges, got %d" % (_abi.MAX_P - 1, edges.size))
        e32 = edges.astype(np.float32)                           # (what the kernels read)
        if not (np.isfinite(e32).all() and (np.diff(e32) > 0).all()):
            raise ValueError("Ordinal: bin edges must be finite and strictly increasing (in float32), got %r" % (edges.tolist(),))
        edges.setflags(write=False)
        return edges

    num_bins = property(lambda self: self.bin_edges.size + 1)

    def _buffer(self):
        if self._buf is None:
            self._buf = torch.tensor([self._sigma_host] + self.bin_edges.tolist(), dtype=settings.float_type, device=settings.default_device())
        return self._buf

    def to(self, device):
        if self._buf is not None:
            self._buf = self._buf.to(device)
        return self

    def host_value(self):
        """sigma's host copy, refreshed from the device buffer when a trainer has moved it since the last read."""
        if self._stale:
            self._sigma_host = float(self._buf[0].item())
            self._stale = False
        return self._sigma_host

    def _set_sigma(self, v):
        if not float(v) > 0.0:
            raise ValueError("Ordinal: sigma must be positive, got %r" % (v,))
        self._sigma_host, self._stale = float(v), False
        if self._buf is not None:
            self._buf[:1].fill_(self._sigma_host)

    sigma = property(host_value, _set_sigma)

    def set_bin_edges(self, bin_edges):
        """New edges of the SAME count, written into the buffer in place (a checkpoint's; a captured graph keeps reading the buffer)."""
        edges = self._checked_edges(bin_edges)
        if edges.size != self.bin_edges.size:
            raise ValueError("Ordinal: %d bin edges cannot replace %d" % (edges.size, self.bin_edges.size))
        self.bin_edges = edges
        if self._buf is not None:
            self._buf[1:].copy_(torch.tensor(edges.tolist(), dtype=settings.float_type))

    # what a trainer needs of DeviceScalarVariance: it takes the view below for its Adam entry, so there is nothing to bind
    def trained_scalar_view(self, device=None):
        """The 1-element view of sigma in the device buffer: a trainer updates it in place and every launch reads it there."""
        if device is not None and self._buffer().device != torch.device(device):
            self.to(device)
        return self._buffer()[:1]

    def bind_device_variance(self, t):
        if t.data_ptr() != self._buffer().data_ptr():
            raise ValueError("Ordinal: sigma lives in the likelihood's own device buffer; train trained_scalar_view()")

    def mark_device_variance_changed(self):
        self._stale = True

    def lik_desc(self):
        d = _abi.LikDesc()
        d.type = _abi.LIK_ORDINAL
        d.param[0], d.param[1] = self._sigma_host, float(self.bin_edges.size)      # (param[0]: possibly stale; it only refuses sigma <= 0)
        d.param0_dev = self._buffer().data_ptr()
        return d

    grad_name = "lik_sigma"

    def trained_scalar(self):
        return self.grad_name, self.sigma

    def check_targets(self, Y):
        """Finite integers in [0, n]: the kernels index the edge array with them (the models call this once on the host when they are built)."""
        import numpy as np
        Yh = _host_targets(Y)
        n = self.bin_edges.size
        _refuse_targets("Ordinal", "integers in [0, %d]" % n, Yh, ~(np.isfinite(Yh) & (Yh >= 0) & (Yh <= n) & (Yh == np.floor(Yh))))


def exp(x):
    """GPflow's default link of ``Poisson`` / ``Exponential`` / ``Gamma`` on torch tensors (the name their ``invlink=...`` accepts)."""
    return torch.exp(x)


def is_gaussian(likelihood):
    """True when the models take the Gaussian routes (the fused tail and heads) for this likelihood: exactly the class above, or an
    object without the protocol that quacks like it (``variance`` / ``desc_variance``, as before the protocol existed)."""
    return isinstance(likelihood, Gaussian) or not hasattr(likelihood, "lik_desc")
