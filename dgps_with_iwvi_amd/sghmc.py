"""The SGHMC inference mode of the reference (experiments/sghmc.py, adapted there from cambridge-mlg/sghmc_dgp; wiring in
experiments/build_models.py:252-261,306-335) on the GPU.

The model is a ``DGP_VI`` (S = 1) whose GP layers all have ``q_sqrt = None``; the sampled tensors theta are the layers' (whitened) ``q_mu``.
One op = one value + gradient evaluation of the bound (``backward.iw_elbo_and_gradients``: the layer launch and the hand-written adjoints;
the full evaluation, although the sampler reads the ``q_mu`` gradients only -- DESIGN.md section 9) and ONE ``iwvi_sghmc_step`` launch over
all sampled tensors (csrc/sghmc.hip): float64 state, Philox noise with the counter on the device.

Reference -> here (no session argument anywhere):
  SGHMC(model, vars, hyper_train_op, window_size)   -> SGHMC(model, window_size, lr=...): vars = every GP layer's q_mu, the hyper op is built in
  generate_update_step(epsilon, mdecay)             -> same name: (re)initialises xi = g = g2 = 1, p = 0
  sample_op / burn_in_op (lists of tf.assign)       -> sample_op() / burn_in_op()
  sghmc_step(session), train_hypers(session)        -> sghmc_step(), train_hypers()
  collect_samples(session, num, spacing)            -> collect_samples(num, spacing): per GP layer a device tensor [num, M, R]
"""
import numpy as np
import torch

from . import _abi, settings
from .backward import iw_elbo_and_gradients
from .layers import GPLayer, LatentVariableLayer
from .temp_workaround import SharedMixedMok

SEED_TAG = 0x5347484D43                                          # "SGHMC": the sampler's Philox key is settings.seed ^ SEED_TAG


class _HyperAdam:
    """TensorFlow AdamOptimizer (``iwvi_adam_step_dev``, the step count on the device) on an entry list of its own: what the reference's
    ``hyper_train_op`` trains in this mode -- every GP layer's Z and lengthscales, the final kernel variance and the likelihood's trained
    scalar (1-element device masters bound to their owners, as ``training.Trainer`` does), W / the linear mean function's A unless
    ``fix_linear``.  q_mu is the sampler's (set_trainable(False), build_models.py:257)."""

    def __init__(self, model, lr, fix_linear, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.lr, self.betas, self.epsilon = float(lr), (beta1, beta2), epsilon
        dev, ft = model.X.device, settings.float_type
        self.entries, self.scalars = [], []
        n = len(model.layers)
        for i, l in enumerate(model.layers):
            k = l._base_kern()
            self.entries.append(("l%d.Z" % i, l._Z(), 0))
            self.entries.append(("l%d.ls" % i, k.lengthscales, 1))
            if i == n - 1:
                t = torch.full((1,), k.variance, dtype=ft, device=dev)
                self.entries.append(("l%d.var" % i, t, 1))
                k.bind_device_variance(t)
                self.scalars.append((t, k))
            if not fix_linear:
                if isinstance(l.kern, SharedMixedMok):
                    self.entries.append(("l%d.W" % i, l.kern.W, 0))
                if l.mean_function.mf_type == _abi.MF_LINEAR:
                    self.entries.append(("l%d.mfA" % i, l.mean_function.A, 0))
        lik = model.likelihood
        lik_par = lik.trained_scalar() if hasattr(lik, "trained_scalar") else ("lik_var", lik.variance)
        if lik_par is not None:
            # (an Ordinal's sigma lives at the head of the likelihood's own device buffer: its view is trained in place)
            t = lik.trained_scalar_view(dev) if hasattr(lik, "trained_scalar_view") else torch.full((1,), lik_par[1], dtype=ft, device=dev)
            self.entries.append((lik_par[0], t, 1))
            lik.bind_device_variance(t)
            self.scalars.append((t, lik))
        for name, t, _ in self.entries:
            _abi.dev_tensor(t, name)
        self.state = [tuple(torch.empty_like(t) for _ in range(3)) for _, t, _ in self.entries]
        self.t_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self._call(None, init=True)

    def _call(self, grads, init=False):
        n = len(self.entries)
        arr = (_abi.AdamTensor * n)()
        keep = []
        for i, ((name, p, tr), (x, m, v)) in enumerate(zip(self.entries, self.state)):
            a = arr[i]
            a.param, a.x, a.m, a.v, a.n, a.transform = p.data_ptr(), x.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), tr
            if not init:
                g = grads[name].reshape(-1)
                if g.dtype == torch.float64:
                    a.transform = tr | _abi.ADAM_GRAD_F64
                g = _abi.dev_tensor(g.contiguous(), "grad " + name, g.dtype)
                if g.numel() != p.numel():
                    raise ValueError("gradient %s has %d entries, parameter has %d" % (name, g.numel(), p.numel()))
                keep.append(g)
                a.grad = g.data_ptr()
        if init:
            _abi.check(_abi.lib().iwvi_adam_step(arr, n, 0.0, self.betas[0], self.betas[1], self.epsilon, 1, 1, 1, _abi.stream_ptr()))
        else:
            _abi.check(_abi.lib().iwvi_adam_step_dev(arr, n, self.lr, self.betas[0], self.betas[1], self.epsilon,
                                                    self.t_dev.data_ptr(), 1, _abi.stream_ptr()))
        return keep

    def step(self, grads):
        self._call(grads)
        for _, owner in self.scalars:
            owner.mark_device_variance_changed()


class SGHMC:
    _STATE = ("xi", "g", "g2", "p", "theta64")

    def __init__(self, model, window_size=100, lr=5e-3, fix_linear=True, use_graph=False, group=None):
        from .models import DGP_IWVI
        import torch.distributed as dist
        # every refusal before any work is queued
        if isinstance(model, DGP_IWVI):
            raise NotImplementedError("SGHMC samples the q_mu of a DGP_VI (S = 1); a DGP_IWVI is not covered (reference build_models.py:252-261)")
        if any(isinstance(l, LatentVariableLayer) for l in model.layers):
            raise NotImplementedError("SGHMC: models with a latent-variable layer are not covered (the reference's grid runs '', G5, G5_G5)")
        if group is not None or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            raise NotImplementedError("SGHMC runs on one rank: sharded groups are not covered")
        if not model.layers or not all(isinstance(l, GPLayer) for l in model.layers):
            raise TypeError("SGHMC needs a stack of GPLayer")
        if any(l.q_sqrt is not None for l in model.layers):
            raise ValueError("SGHMC needs q_sqrt = None on every GP layer (build_models.build_sghmc_model builds such a model)")
        if int(window_size) < 1:
            raise ValueError("window_size must be >= 1")
        if len(model.layers) > _abi.SGHMC_MAX_TENSORS:
            raise ValueError("more than %d sampled tensors" % _abi.SGHMC_MAX_TENSORS)
        self.model = model
        self.layers = list(model.layers)
        self.vars = [l.q_mu for l in self.layers]                # (the reference's name) the layers' OWN buffers, updated in place
        for t in self.vars:
            _abi.dev_tensor(t, "q_mu")
        self.window_size = int(window_size)
        self.use_graph = bool(use_graph)
        dev = model.X.device
        self.window = [torch.zeros(self.window_size, *t.shape, dtype=t.dtype, device=dev) for t in self.vars]   # device ring buffer per layer
        self.window_len, self._window_pos = 0, 0
        self._choice = np.random.RandomState(0)                  # which window member the hyper step sees (reference: np.random.randint)
        self.adam = _HyperAdam(model, lr, fix_linear)
        self.rng_state = torch.zeros(2, dtype=torch.int64, device=dev)     # {Philox counter, arrival ticket} of the sampler's noise stream
        self.epsilon = self.mdecay = None
        self.state = None
        self.sample_op_count = self.burn_in_op_count = self.hyper_step_count = 0
        self._graphs = {}
        self._cap_stream = None
        self._capturing = False

    # -- the sampler ---------------------------------------------------------------------------
    def generate_update_step(self, epsilon, mdecay):
        """sghmc.py:19-54: the step sizes and a fresh sampler state (xi = g = g2 = 1, p = 0; the float64 master of theta from q_mu)."""
        if not (epsilon > 0.0) or not (mdecay >= 0.0):
            raise ValueError("epsilon > 0 and mdecay >= 0 expected, got %r, %r" % (epsilon, mdecay))
        self.epsilon, self.mdecay = float(epsilon), float(mdecay)
        self.state = []
        for t in self.vars:
            one = torch.ones(t.shape, dtype=torch.float64, device=t.device)
            self.state.append(dict(xi=one.clone(), g=one.clone(), g2=one.clone(), p=torch.zeros_like(one), theta64=t.double()))
        self._graphs = {}                                        # the scalars enter the launch by value
        return self

    def _seed(self):
        return (int(settings.seed) ^ SEED_TAG) & 0xFFFFFFFFFFFFFFFF

    def _update(self, grads, burn_in, noise=None, noise_out=None):
        """ONE ``iwvi_sghmc_step`` launch over every layer's q_mu."""
        n = len(self.vars)
        arr = (_abi.SghmcTensor * n)()
        keep = []
        for i, (t, st) in enumerate(zip(self.vars, self.state)):
            a = arr[i]
            g = _abi.dev_tensor(grads["l%d.q_mu" % i].reshape(-1).contiguous(), "grad l%d.q_mu" % i)
            if g.numel() != t.numel():
                raise ValueError("gradient l%d.q_mu has %d entries, q_mu has %d" % (i, g.numel(), t.numel()))
            a.theta, a.grad, a.n = t.data_ptr(), g.data_ptr(), t.numel()
            a.xi, a.g, a.g2, a.p, a.theta64 = (st[k].data_ptr() for k in self._STATE)
            keep.append(g)
            if noise is not None and noise[i] is not None:
                z = _abi.dev_tensor(noise[i].reshape(-1).contiguous(), "noise")
                if z.numel() != t.numel():
                    raise ValueError("noise[%d] has %d entries, q_mu has %d" % (i, z.numel(), t.numel()))
                a.noise = z.data_ptr()
                keep.append(z)
            if noise_out is not None and noise_out[i] is not None:
                zo = _abi.dev_tensor(noise_out[i], "noise_out")
                if zo.numel() != t.numel():
                    raise ValueError("noise_out[%d] has %d entries, q_mu has %d" % (i, zo.numel(), t.numel()))
                a.noise_out = zo.data_ptr()
        _abi.check(_abi.lib().iwvi_sghmc_step(arr, n, self.epsilon, self.mdecay, float(self.model.num_data), 1 if burn_in else 0,
                                              self._seed(), self.rng_state.data_ptr(), _abi.stream_ptr()))
        return keep

    def _evaluate_and_update(self, burn_in, zs=None, noise=None, noise_out=None):
        elbo, g = iw_elbo_and_gradients(self.model, zs, mode_vi=True)
        self._update(g, burn_in, noise, noise_out)
        return elbo

    def _op(self, burn_in, zs, noise, noise_out):
        if self.state is None:
            raise RuntimeError("call generate_update_step(epsilon, mdecay) first (model.init_op() does)")
        name = "burn_in" if burn_in else "sample"
        if self.use_graph:
            if zs is not None or noise is not None or noise_out is not None:
                raise ValueError("use_graph draws the noise on the device (a captured graph takes no per-step host arguments)")
            self.model.next_minibatch()                          # host-driven: outside the graph, into the same X / Y buffers
            elbo = self._replay(name, lambda: self._evaluate_and_update(burn_in))
        else:
            self.model.next_minibatch()                          # a new minibatch per session.run (models.py:21-26)
            elbo = self._evaluate_and_update(burn_in, zs, noise, noise_out)
        if burn_in:
            self.burn_in_op_count += 1
        else:
            self.sample_op_count += 1
        return elbo

    def sample_op(self, zs=None, noise=None, noise_out=None):
        """One sampler step that writes theta and p only (sghmc.py:53).  ``zs``: the layers' noise ([N, dim] each, S = 1) or None -> drawn in
        the layer kernel; ``noise``: per layer the update's N(0, 1) draws [M, R] or None -> drawn in the update kernel; ``noise_out``: per layer a
        [M, R] buffer that receives what was used.  Returns the bound (0-dim float64 device tensor)."""
        return self._op(False, zs, noise, noise_out)

    def burn_in_op(self, zs=None, noise=None, noise_out=None):
        """The same step, also writing xi, g, g2 (sghmc.py:54)."""
        return self._op(True, zs, noise, noise_out)

    def _replay(self, name, op):
        """Capture ``op`` into a hipGraph on first use (after one eager run, which is this call's step), then replay it; captured again when a
        layer's arithmetic route moves (``model.route_key()``)."""
        key = self.model.route_key()
        ent = self._graphs.get(name)
        if ent is not None and ent[0] == key:
            ent[1].replay()
            return ent[2]
        self._capturing = True
        try:
            if self._cap_stream is None:
                self._cap_stream = torch.cuda.Stream(device=self.model.X.device)
            side = self._cap_stream
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                eager = op()                                     # this call's step (it also warms the allocator pools)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                    elbo = op()                                  # recorded, not executed
            torch.cuda.current_stream().wait_stream(side)
        finally:
            self._capturing = False
        self._graphs[name] = (key, g, elbo)
        return eager

    # -- the reference's training step -----------------------------------------------------------
    def sghmc_step(self, zs=None, noise=None):
        """sghmc.py:69-77: one burn-in op, then the current theta joins the window of the last ``window_size``."""
        elbo = self.burn_in_op(zs, noise)
        for w, t in zip(self.window, self.vars):
            w[self._window_pos].copy_(t)
        self._window_pos = (self._window_pos + 1) % self.window_size
        self.window_len = min(self.window_len + 1, self.window_size)
        return elbo

    def train_hypers(self, zs=None):
        """sghmc.py:79-83: one Adam step on every other trainable parameter, evaluated with theta replaced by a uniformly drawn member of
        the window.  The chain's own theta is back, bit for bit, when this returns."""
        if self.window_len == 0:
            raise RuntimeError("the window is empty: call sghmc_step() first")
        i = int(self._choice.randint(self.window_len))
        for w, t in zip(self.window, self.vars):
            t.copy_(w[i])
        self.model.next_minibatch()
        elbo, g = iw_elbo_and_gradients(self.model, zs, mode_vi=True)
        self.adam.step(g)
        for t, st in zip(self.vars, self.state):
            t.copy_(st["theta64"])                               # theta is the float32 rounding of its master: restored exactly
        self.hyper_step_count += 1
        return elbo

    def collect_samples(self, num, spacing):
        """sghmc.py:56-67: ``num`` kept theta, ``spacing`` sample ops in front of each -> per GP layer a device tensor [num, M, R]."""
        num, spacing = int(num), int(spacing)
        if num < 1 or spacing < 1:
            raise ValueError("num and spacing must be >= 1")
        out = [torch.empty(num, *t.shape, dtype=t.dtype, device=t.device) for t in self.vars]
        for k in range(num):
            for _ in range(spacing):
                self.sample_op()
            for o, t in zip(out, self.vars):
                o[k].copy_(t)
        return out

    # -- checkpoint ------------------------------------------------------------------------------
    def state_dict(self):
        """Sampler state, window, Adam state and every counter, as CPU arrays (the model's own parameters, minibatch position and layer-noise
        counter are ``build_models.state_dict(model)``'s)."""
        if self.state is None:
            raise RuntimeError("no sampler state yet: call generate_update_step first")
        out = {"epsilon": np.float64(self.epsilon), "mdecay": np.float64(self.mdecay),
               "window_len": np.int64(self.window_len), "window_pos": np.int64(self._window_pos),
               "rng_counter": np.int64(int(self.rng_state[0].item())), "adam_t": np.int64(int(self.adam.t_dev.item())),
               "counts": np.array([self.sample_op_count, self.burn_in_op_count, self.hyper_step_count], dtype=np.int64)}
        kind, keys, pos, has_gauss, cached = self._choice.get_state()
        out["choice.keys"], out["choice.pos"] = np.asarray(keys), np.int64(pos)
        for i, (st, w) in enumerate(zip(self.state, self.window)):
            for k in self._STATE:
                out["l%d.%s" % (i, k)] = st[k].detach().cpu().numpy()
            out["l%d.window" % i] = w.detach().cpu().numpy()
        for (name, _, _), (x, m, v) in zip(self.adam.entries, self.adam.state):
            out["adam.x." + name], out["adam.m." + name], out["adam.v." + name] = (a.detach().cpu().numpy() for a in (x, m, v))
        return out

    def load_state_dict(self, state):
        """After the model's parameters have been restored in place (``build_models.load_state_dict``)."""
        self.generate_update_step(float(state["epsilon"]), float(state["mdecay"]))
        self.window_len, self._window_pos = int(state["window_len"]), int(state["window_pos"])
        self.rng_state[0] = int(state["rng_counter"])
        self.rng_state[1] = 0
        self.adam.t_dev.fill_(int(state["adam_t"]))
        self.sample_op_count, self.burn_in_op_count, self.hyper_step_count = (int(c) for c in np.asarray(state["counts"]))
        self._choice.set_state(("MT19937", np.asarray(state["choice.keys"], dtype=np.uint32), int(state["choice.pos"]), 0, 0.0))
        put = lambda dst, a: dst.copy_(torch.as_tensor(np.asarray(a), dtype=dst.dtype, device=dst.device).reshape(dst.shape))
        for i, (st, w, t) in enumerate(zip(self.state, self.window, self.vars)):
            for k in self._STATE:
                put(st[k], state["l%d.%s" % (i, k)])
            put(w, state["l%d.window" % i])
            t.copy_(st["theta64"])
        for (name, _, _), (x, m, v) in zip(self.adam.entries, self.adam.state):
            for key, dst in (("adam.x.", x), ("adam.m.", m), ("adam.v.", v)):
                put(dst, state[key + name])
        self._graphs = {}
        return self
