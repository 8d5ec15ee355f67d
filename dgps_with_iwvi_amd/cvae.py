"""The CVAE baseline of the reference (experiments/build_models.py:29-142, its wiring :148-173) on the GPU: an MLP encoder and an MLP decoder in
float32 with one Gaussian observation variance, trained by Adam on the minibatch bound

    elbo = sum_{n,d} log N(y_nd; decoder(z_n, x_n)_d, variance) - sum_{n,j} KL(N(mu_nj, sigma_nj^2) || N(0, 1)),   z = mu + eps sigma.

Value and gradient are two launches of csrc/cvae.hip (``iwvi_cvae_elbo_and_grad``), a predictive sample set one (``iwvi_cvae_predict_samples``);
Adam is ``iwvi_adam_step_dev`` over every weight, every bias and the variance.  There is no torch fallback: off the GPU the compute methods raise.

Three behaviours of the reference are kept on purpose: the bound carries no N / B scale; ``predict_y`` returns ONE decoder
draw per row as its "mean"; the learning rate decays by a fixed 0.98 per 1000 steps whatever ``ARGS.lr_decay`` says.

Reference -> here:
  CVAE(X, Y, latent_dim, layers, batch_size, name)   -> same signature (plus ``device`` and ``rng`` for the initial values)
  model.Ws / bs / Ws_dec / bs_dec / variance         -> lists of device tensors; ``variance`` reads the host copy of ``variance_dev``
  compute_log_likelihood(), predict_y, predict_y_samples (autoflow) -> methods without a session
"""
import ctypes

import numpy as np
import torch

from . import _abi, settings
from .likelihoods import Gaussian
from .training import staircase_decay

SEED_TAG = 0x43564145                                            # "CVAE": the model's Philox key is settings.seed ^ SEED_TAG


class CVAE:
    _PREDICT_ROWS = 1 << 24                                      # default cap on N x S rows per sampling launch (the kernel takes < 2^31)

    def __init__(self, X, Y, latent_dim, layers, batch_size=64, name=None, device=None, rng=None, activation=_abi.ACT_TANH):
        rng = np.random if rng is None else rng
        dev = torch.device(device) if device is not None else settings.default_device()
        X, Y = np.asarray(X, dtype=np.float32), np.asarray(Y, dtype=np.float32)
        if X.ndim != 2 or Y.ndim != 2 or X.shape[0] != Y.shape[0]:
            raise ValueError("X [N, Dx] and Y [N, Dy] expected, got %s and %s" % (X.shape, Y.shape))
        self.X_dim, self.Y_dim, self.latent_dim = X.shape[1], Y.shape[1], int(latent_dim)
        self.layers_widths = [int(w) for w in layers]
        self.enc_dims = [self.X_dim + self.Y_dim] + self.layers_widths + [2 * self.latent_dim]
        self.dec_dims = [self.latent_dim + self.X_dim] + self.layers_widths + [self.Y_dim]
        if len(self.enc_dims) - 1 > _abi.CVAE_MAX_MAPS or max(self.enc_dims + self.dec_dims) > _abi.CVAE_MAX_WIDTH or min(self.enc_dims + self.dec_dims) < 1:
            raise ValueError("at most %d linear maps per net and widths 1 .. %d (Dx + Dy and L + Dx included), got %s / %s"
                             % (_abi.CVAE_MAX_MAPS, _abi.CVAE_MAX_WIDTH, self.enc_dims, self.dec_dims))
        if not 1 <= self.latent_dim <= _abi.CVAE_MAX_L or not 1 <= self.Y_dim <= _abi.CVAE_MAX_DY:
            raise ValueError("latent_dim 1 .. %d and Dy 1 .. %d expected" % (_abi.CVAE_MAX_L, _abi.CVAE_MAX_DY))
        self.activation = int(activation)
        self.num_data = X.shape[0]
        self.batch_size = batch_size
        self.name = name
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev).contiguous()
        self._X_all, self._Y_all = t(X), t(Y)
        self.X, self.Y = self._X_all, self._Y_all

        def net(dims):                                           # W ~ N(0, 2 / (in + out)), b = 0 (:56-61, :77-82)
            Ws = [t(rng.randn(i, o) * (2.0 / (i + o)) ** 0.5) for i, o in zip(dims[:-1], dims[1:])]
            return Ws, [torch.zeros(o, dtype=torch.float32, device=dev) for o in dims[1:]]
        # (the reference builds the encoder first, then the decoder: the same order of draws from the host generator)
        self.Ws, self.bs = net(self.enc_dims)
        self.Ws_dec, self.bs_dec = net(self.dec_dims)
        self.likelihood = Gaussian(0.05)                         # Parameter(.05, transform=positive) (:44)
        self.variance_dev = torch.full((1,), 0.05, dtype=torch.float32, device=dev)
        self.likelihood.bind_device_variance(self.variance_dev)
        self._mb_rng = np.random.RandomState(0)                  # Minibatch(seed=0)
        self._mb_perm, self._mb_pos = None, 0
        self.rng_state = torch.zeros(2, dtype=torch.int64, device=dev)   # {Philox counter, arrival ticket}
        self._ws, self._grads = {}, None
        if batch_size is not None:
            self.next_minibatch()

    # -- what evaluation.py asks of a model ----------------------------------------------------
    def _output_dim(self):
        return self.Y_dim

    def _input_dim(self):
        return self.X_dim

    @property
    def variance(self):
        return self.likelihood.variance

    @variance.setter
    def variance(self, v):
        self.likelihood.variance = v

    # -- data (the iterator of models.DGP_VI.next_minibatch: shuffled epochs, the same buffers on every step) --
    def next_minibatch(self):
        if self.batch_size is None:
            return
        n = self._X_all.shape[0]
        b = min(self.batch_size, n)
        if self._mb_perm is None or self._mb_pos + b > n:
            self._mb_perm = torch.as_tensor(self._mb_rng.permutation(n), device=self._X_all.device)
            self._mb_pos = 0
        idx = self._mb_perm[self._mb_pos:self._mb_pos + b]
        self._mb_pos += b
        if self.X.shape[0] == b and self.X.data_ptr() != self._X_all.data_ptr():
            torch.index_select(self._X_all, 0, idx, out=self.X)
            torch.index_select(self._Y_all, 0, idx, out=self.Y)
        else:
            self.X, self.Y = self._X_all[idx].contiguous(), self._Y_all[idx].contiguous()

    def parameters(self):
        """[(name, tensor)]: every weight, every bias, the variance -- the order of the gradients and of the optimiser's entries."""
        out = []
        for tag, Ws, bs in (("enc", self.Ws, self.bs), ("dec", self.Ws_dec, self.bs_dec)):
            for i, (w, b) in enumerate(zip(Ws, bs)):
                out += [("%s_W%d" % (tag, i), w), ("%s_b%d" % (tag, i), b)]
        return out + [("variance", self.variance_dev)]

    # -- the C-ABI ------------------------------------------------------------------------------
    def _seed(self):
        return (int(settings.seed) ^ SEED_TAG) & 0xFFFFFFFFFFFFFFFF

    def _desc(self):
        """(iwvi_cvae_desc, the ctypes arrays it points into)."""
        for name, p in self.parameters():
            _abi.dev_tensor(p, name)
        n = len(self.Ws)
        keep = [_abi.ptr_array(self.Ws), _abi.ptr_array(self.bs), _abi.ptr_array(self.Ws_dec), _abi.ptr_array(self.bs_dec),
                (ctypes.c_int32 * (n + 1))(*self.enc_dims), (ctypes.c_int32 * (n + 1))(*self.dec_dims)]
        d = _abi.CvaeDesc()
        d.enc_W, d.enc_b, d.dec_W, d.dec_b, d.enc_dims, d.dec_dims = keep
        d.n_maps, d.Dx, d.Dy, d.L, d.act = n, self.X_dim, self.Y_dim, self.latent_dim, self.activation
        d.variance, d.variance_dev = 0.05, self.variance_dev.data_ptr()      # the device scalar wins
        return d, keep

    def _workspace(self, d, B):
        ws = self._ws.get(B)
        if ws is None:
            nbytes = _abi.lib().iwvi_cvae_ws_bytes(ctypes.byref(d), B)
            ws = self._ws[B] = torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=self.X.device)
        return ws

    def _eps(self, eps, B):
        if eps is None:
            return None
        eps = _abi.dev_tensor(eps, "eps")
        if tuple(eps.shape) != (B, self.latent_dim):
            raise ValueError("eps must be [%d, %d], got %s" % (B, self.latent_dim, tuple(eps.shape)))
        return eps

    def gradient_buffers(self):
        """The tensors ``elbo_and_gradients`` writes, by parameter name -- the same ones on every call (a captured graph keeps writing
        them); ``variance`` is float64 [1]."""
        if self._grads is None:
            self._grads = {name: torch.zeros_like(p) for name, p in self.parameters()[:-1]}
            self._grads["variance"] = torch.zeros(1, dtype=torch.float64, device=self.X.device)
        return self._grads

    def compute_log_likelihood(self, eps=None, eps_out=None, parts=False):
        """The minibatch bound (0-dim float64 device tensor; ``parts``: the [3] tensor (elbo, sum log p, sum KL)).  ``eps`` [B, L] or None ->
        drawn in the launch from the model's device counter; ``eps_out`` [B, L] receives what was used."""
        X, Y = _abi.dev_tensor(self.X, "X"), _abi.dev_tensor(self.Y, "Y")
        B = X.shape[0]
        eps = self._eps(eps, B)
        d, keep = self._desc()
        out = torch.empty(3, dtype=torch.float64, device=X.device)
        _abi.check(_abi.lib().iwvi_cvae_elbo(ctypes.byref(d), _abi.ptr(X), _abi.ptr(Y), B, _abi.ptr(eps), self._seed(),
                                             _abi.ptr(self.rng_state), _abi.ptr(eps_out), _abi.ptr(out), _abi.ptr(self._workspace(d, B)),
                                             _abi.stream_ptr()))
        return out if parts else out[0]

    def elbo_and_gradients(self, eps=None, eps_out=None, parts=False):
        """-> (bound, {name: d bound / d parameter}) in two launches; the gradients are ``gradient_buffers()``."""
        X, Y = _abi.dev_tensor(self.X, "X"), _abi.dev_tensor(self.Y, "Y")
        B = X.shape[0]
        eps = self._eps(eps, B)
        d, keep = self._desc()
        g = self.gradient_buffers()
        n = len(self.Ws)
        arrs = [_abi.ptr_array([g["%s_%s%d" % (tag, kind, i)] for i in range(n)]) for tag in ("enc", "dec") for kind in ("W", "b")]
        gd = _abi.CvaeGrads()
        gd.enc_dW, gd.enc_db, gd.dec_dW, gd.dec_db = arrs
        gd.dvariance = g["variance"].data_ptr()
        out = torch.empty(3, dtype=torch.float64, device=X.device)
        _abi.check(_abi.lib().iwvi_cvae_elbo_and_grad(ctypes.byref(d), _abi.ptr(X), _abi.ptr(Y), B, _abi.ptr(eps), self._seed(),
                                                      _abi.ptr(self.rng_state), _abi.ptr(eps_out), _abi.ptr(out), ctypes.byref(gd),
                                                      _abi.ptr(self._workspace(d, B)), _abi.stream_ptr()))
        return (out if parts else out[0]), g

    def _sample(self, Xs, S, flags, z=None, z_y=None, batch_size=None):
        dev = self.X.device
        Xs = torch.as_tensor(np.asarray(Xs, dtype=np.float32), device=dev) if not isinstance(Xs, torch.Tensor) else Xs.to(dev, torch.float32)
        Xs = _abi.dev_tensor(Xs.contiguous(), "Xs")
        if Xs.dim() != 2 or Xs.shape[1] != self.X_dim:
            raise ValueError("Xs must be [N, %d], got %s" % (self.X_dim, tuple(Xs.shape)))
        N, S = Xs.shape[0], int(S)
        if N < 1 or S < 1:
            raise ValueError("N >= 1 and S >= 1 expected")
        out = torch.empty(N, S, self.Y_dim, dtype=torch.float32, device=dev)
        bs = max(1, self._PREDICT_ROWS // S) if batch_size is None else int(batch_size)
        if bs < 1:
            raise ValueError("batch_size must be >= 1")
        d, keep = self._desc()
        for lo in range(0, N, bs):
            n = min(bs, N - lo)
            zz = None if z is None else _abi.dev_tensor(z[lo:lo + n].contiguous(), "z")
            zy = None if z_y is None else _abi.dev_tensor(z_y[lo:lo + n].contiguous(), "z_y")
            _abi.check(_abi.lib().iwvi_cvae_predict_samples(ctypes.byref(d), _abi.ptr(Xs[lo:lo + n]), n, S, _abi.ptr(zz), _abi.ptr(zy), flags,
                                                            self._seed(), _abi.ptr(self.rng_state), _abi.ptr(out[lo:lo + n]),
                                                            _abi.stream_ptr()))
        return out

    def predict_y(self, Xs):
        """(:123-130) one z ~ N(0, 1) per row -> (decoder(z, Xs), sqrt(variance) 1): the "mean" is itself a draw, as in the reference."""
        y = self._sample(Xs, 1, _abi.CVAE_NO_Y_NOISE)[:, 0, :]
        return y, torch.ones_like(y) * self.variance_dev.sqrt()

    def predict_y_samples_fused(self, Xs, S, z=None, z_y=None, batch_size=None):
        """(:132-142) [S, N, Dy] = decoder(z, x_n) + sqrt(variance) eps', z and eps' fresh for every (s, n): a view of the [N, S, Dy] the
        launch writes (a point's S samples contiguous).  z [N, S, L] / z_y [N, S, Dy]: injected draws."""
        return self._sample(Xs, S, 0, z, z_y, batch_size).permute(1, 0, 2)

    def predict_y_samples(self, Xs, S):
        return self.predict_y_samples_fused(Xs, S)

    # -- checkpoint --------------------------------------------------------------------------------
    def state_dict(self):
        out = {"cvae." + name: p.detach().cpu().numpy() for name, p in self.parameters()}
        kind, keys, pos, has_gauss, cached = self._mb_rng.get_state()
        out["minibatch.rng_keys"], out["minibatch.rng_pos"], out["minibatch.pos"] = np.asarray(keys), np.int64(pos), np.int64(self._mb_pos)
        if self._mb_perm is not None:
            out["minibatch.perm"] = self._mb_perm.detach().cpu().numpy()
        out["rng.counter"] = np.int64(int(self.rng_state[0].item()))
        out["rng.seed"] = np.int64(settings.seed)
        return out

    def load_state_dict(self, state):
        """In place: a trainer built on the model keeps pointing at live tensors."""
        for name, p in self.parameters():
            p.copy_(torch.as_tensor(np.asarray(state["cvae." + name]), dtype=p.dtype, device=p.device).reshape(p.shape))
        self.likelihood.mark_device_variance_changed()
        if "minibatch.rng_keys" in state:
            self._mb_rng.set_state(("MT19937", np.asarray(state["minibatch.rng_keys"], dtype=np.uint32), int(state["minibatch.rng_pos"]), 0, 0.0))
            self._mb_pos = int(state["minibatch.pos"])
            self._mb_perm = (torch.as_tensor(np.asarray(state["minibatch.perm"]), device=self.X.device) if "minibatch.perm" in state else None)
            if self.batch_size is not None and self._mb_perm is not None and self._mb_pos > 0:
                b = min(self.batch_size, self._X_all.shape[0])
                idx = self._mb_perm[self._mb_pos - b:self._mb_pos]
                self.X.copy_(self._X_all[idx])
                self.Y.copy_(self._Y_all[idx])
        if "rng.counter" in state:
            self.rng_state[0] = int(state["rng.counter"])
            self.rng_state[1] = 0
            settings.seed = int(state["rng.seed"])
        return self


class CVAETrainer:
    """The reference's train op (:163-171): global_step += 1, then one Adam step on every weight, every bias and the variance at the rate
    lr 0.98^floor(global_step / 1000).  The reference runs the two ops in one ``session.run``, which leaves their order open; here the
    increment comes first, as in ``training.Trainer``.  ``use_graph=True`` replays value + gradient + Adam as one hipGraph: fresh noise
    comes from the model's device counter, the minibatch gather stays outside the graph, and the graph is captured again when the
    staircase moves the rate (it enters the update by value)."""
    DECAY, EVERY = 0.98, 1000

    def __init__(self, model, lr=5e-3, use_graph=False, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.model, self.lr, self.betas, self.epsilon = model, float(lr), (beta1, beta2), epsilon
        self.use_graph = bool(use_graph)
        self.global_step = 0
        self.entries = [(name, p, 1 if name == "variance" else 0) for name, p in model.parameters()]
        for name, p, _ in self.entries:
            _abi.dev_tensor(p, name)
        self.state = [tuple(torch.empty_like(p) for _ in range(3)) for _, p, _ in self.entries]
        self.t_dev = torch.zeros(1, dtype=torch.int64, device=model.X.device)
        self._graph, self._cap_stream = None, None
        _abi.check(_abi.lib().iwvi_adam_step(self._tensors(None), len(self.entries), 0.0, self.betas[0], self.betas[1], self.epsilon,
                                             1, 1, 1, _abi.stream_ptr()))

    def learning_rate(self):
        return staircase_decay(self.lr, self.global_step, self.DECAY, self.EVERY)

    def _tensors(self, grads):
        arr = (_abi.AdamTensor * len(self.entries))()
        for a, (name, p, tr), (x, m, v) in zip(arr, self.entries, self.state):
            a.param, a.x, a.m, a.v, a.n, a.transform = p.data_ptr(), x.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), tr
            if grads is not None:
                g = grads[name]
                if g.dtype == torch.float64:
                    a.transform = tr | _abi.ADAM_GRAD_F64
                a.grad = g.data_ptr()
        return arr

    def _evaluate_and_update(self, eps, lr):
        elbo, g = self.model.elbo_and_gradients(eps)
        _abi.check(_abi.lib().iwvi_adam_step_dev(self._tensors(g), len(self.entries), lr, self.betas[0], self.betas[1], self.epsilon,
                                                 self.t_dev.data_ptr(), 1, _abi.stream_ptr()))
        return elbo

    def step(self, eps=None):
        """One ``train_op``; returns the bound the step saw (0-dim float64 device tensor)."""
        self.global_step += 1
        lr = self.learning_rate()
        self.model.next_minibatch()                              # host-driven: outside the graph, into the same X / Y buffers
        if self.use_graph:
            if eps is not None:
                raise ValueError("use_graph draws the noise on the device (a captured graph takes no per-step host arguments)")
            elbo = self._replay(lr)
        else:
            elbo = self._evaluate_and_update(eps, lr)
        self.model.likelihood.mark_device_variance_changed()
        return elbo

    def _replay(self, lr):
        key = (self.global_step // self.EVERY, self.model.X.data_ptr(), self.model.X.shape[0])
        ent = self._graph
        if ent is not None and ent[0] == key:
            ent[1].replay()
            return ent[2]
        if self._cap_stream is None:
            self._cap_stream = torch.cuda.Stream(device=self.model.X.device)
        side = self._cap_stream
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eager = self._evaluate_and_update(None, lr)          # this call's step (it also sizes the workspace and the gradient buffers)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                elbo = self._evaluate_and_update(None, lr)       # recorded, not executed
        torch.cuda.current_stream().wait_stream(side)
        self._graph = (key, g, elbo)
        return eager

    def state_dict(self):
        out = {"global_step": np.int64(self.global_step), "adam_t": np.int64(int(self.t_dev.item()))}
        for (name, _, _), (x, m, v) in zip(self.entries, self.state):
            out["x." + name], out["m." + name], out["v." + name] = (a.detach().cpu().numpy() for a in (x, m, v))
        return out

    def load_state_dict(self, state):
        """After the model's parameters have been restored in place."""
        self.global_step = int(state["global_step"])
        self.t_dev.fill_(int(state["adam_t"]))
        self._graph = None
        for (name, _, _), (x, m, v) in zip(self.entries, self.state):
            for key, dst in (("x.", x), ("m.", m), ("v.", v)):
                dst.copy_(torch.as_tensor(np.asarray(state[key + name]), dtype=dst.dtype, device=dst.device).reshape(dst.shape))
        return self
