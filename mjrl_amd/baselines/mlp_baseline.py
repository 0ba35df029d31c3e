"""MLP value baseline with the API of mjrl/baselines/mlp_baseline.py:15-115, fitted
and evaluated on the GPU.

Same model as the reference: Linear(n+4, 128) - ReLU - Linear(128, 128) - ReLU -
Linear(128, 1) on [clip(obs, +-10) / 10, (t/1000)^1..4] features (f32), created in
the reference's module order (so a torch.manual_seed gives the same initial
weights), trained by minibatch Adam (lr, weight_decay = reg_coef) on MSE for
`epochs` passes, minibatches drawn from numpy's global RNG exactly as
mlp_baseline.py:83-96 does (one np.random.permutation per epoch,
int(N / batch_size) - 1 minibatches).

Unlike the reference module, importing this one changes no environment variable
(mlp_baseline.py:1-5 sets CUDA_VISIBLE_DEVICES = '0', which would hide GPUs 1-7
of a multi-GPU run).

Device work: the features are built on the GPU, every minibatch step (gather,
forward, MSE, backward, Adam) is one replay of a captured hipGraph that reads
the minibatch rows through a device index buffer (hipBLAS GEMMs inside), and
predict is one forward.  The CPU model stays the source of truth for pickling and
CPU sampling: its parameters and Adam state are copied to the device before a
fit and back after it.  Sharded (fit_sharded, one process per GPU): rank 0's
permutation is broadcast, every rank computes the minibatch gradient over its
own rows of each minibatch, the gradients are all-reduced (a sum: the MSE is a
mean over the global minibatch), and every rank takes the same Adam step.

fit_backend = "hip" (opt-in, per instance or on the class) replaces the graph
replays of fit / fit_features_device by the hand-written kernels of
csrc/value_fit.hip: one mjrl_value_mlp_epoch call per epoch on the device
model's own parameters and the device optimizer's moments, the same permutation
buffer, batch_size <= 64.  The sharded fit stays on torch
whatever the attribute says.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _device_fit as _fit
from .. import _lib
from .._device_fit import FIT_BACKENDS, HIP_MAX_BATCH


def _features_np(paths, n):
    """mlp_baseline.py:37-56 on the host (f64, as the reference builds it)."""
    o = np.concatenate([p["observations"] for p in paths])
    o = np.clip(o, -10, 10) / 10.0
    if o.ndim > 2:
        o = o.reshape(o.shape[0], -1)
    N = o.shape[0]
    feat = np.ones((N, n + 4))
    feat[:, :n] = o
    k = 0
    for p in paths:
        H = len(p["rewards"])
        al = np.arange(H) / 1000.0
        for j in range(4):
            feat[k:k + H, -4 + j] = al ** (j + 1)
        k += H
    return feat


class MLPBaseline:
    # "torch": a captured graph of torch ops per minibatch step; "hip": the fused
    # kernels of csrc/value_fit.hip (fit / fit_features_device only)
    fit_backend = "torch"

    def __init__(self, env_spec, obs_dim=None, learn_rate=1e-3, reg_coef=0.0, batch_size=64, epochs=1,
                 use_gpu=False, device=None):
        self.n = obs_dim if obs_dim is not None else env_spec.observation_dim
        self.batch_size = batch_size
        self.epochs = epochs
        self.reg_coef = reg_coef
        self.use_gpu = use_gpu   # kept for API parity: fit / predict run on the GPU whenever one is visible
        self.learn_rate = learn_rate
        self.model = nn.Sequential()
        self.model.add_module("fc_0", nn.Linear(self.n + 4, 128))
        self.model.add_module("relu_0", nn.ReLU())
        self.model.add_module("fc_1", nn.Linear(128, 128))
        self.model.add_module("relu_1", nn.ReLU())
        self.model.add_module("fc_2", nn.Linear(128, 1))
        self.optimizer = torch.optim.Adam(self.model.parameters(), lr=learn_rate, weight_decay=reg_coef)
        self.loss_function = torch.nn.MSELoss()
        self._device = device
        self._dev = None   # device mirror (never pickled)

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_dev"] = None
        return d

    def _features(self, paths):
        return _features_np(paths, self.n)

    # ---- device mirror -----------------------------------------------------
    def _device_of(self):
        if self._device is not None:
            return torch.device(self._device)
        return torch.device("cuda", torch.cuda.current_device())

    def _to_device(self):
        """Device copies of the model and of the Adam state (the CPU objects stay
        the source of truth between fits)."""
        dev = self._device_of()
        st = self._dev
        if st is None or st["device"] != dev:
            model = nn.Sequential(
                nn.Linear(self.n + 4, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, 1)).to(dev)
            opt = torch.optim.Adam(model.parameters(), lr=self.learn_rate, weight_decay=self.reg_coef,
                                   capturable=True)
            st = self._dev = dict(device=dev, model=model, opt=opt, graph=None)
        model, opt = st["model"], st["opt"]
        with torch.no_grad():
            for pd, pc in zip(model.parameters(), self.model.parameters()):
                pd.copy_(pc.data)
        _fit.state_to_device(self.optimizer, list(self.model.parameters()), opt, list(model.parameters()), dev, True)
        st["cpu_key"] = self._cpu_key()
        return st

    def _cpu_key(self):
        """Identity of the CPU parameters' current contents: their storage (a
        `param.data = ...` assignment changes it) and the parameters' version
        counters (in-place updates through the parameter, e.g. an optimizer
        step).  Edits through `param.data.<op>_()` bypass the counter and are not
        seen."""
        return tuple((p.data_ptr(), p._version) for p in self.model.parameters())

    def _predict_state(self):
        """The device mirror for a forward: re-copied when the CPU parameters
        changed since the last copy (a caller may set them directly)."""
        st = self._dev
        if st is None or st.get("cpu_key") != self._cpu_key():
            st = self._to_device()
        return st

    def _from_device(self, st):
        model, opt = st["model"], st["opt"]
        with torch.no_grad():
            for pd, pc in zip(model.parameters(), self.model.parameters()):
                pc.data.copy_(pd.detach().cpu())
        st["cpu_key"] = self._cpu_key()
        _fit.state_to_cpu(self.optimizer, list(self.model.parameters()), opt, list(model.parameters()))

    def _step_graph(self, st, X, Y):
        """One minibatch Adam step as a captured hipGraph over static buffers:
        idx (the minibatch row indices) -> gather -> forward -> MSE -> backward
        -> Adam.  Captured once per (X, Y) buffers."""
        key = (X.data_ptr(), Y.data_ptr(), X.shape[0], self.batch_size)
        if st["graph"] is not None and st["gkey"] == key:
            return st
        model, opt = st["model"], st["opt"]
        dev = st["device"]
        idx = torch.zeros(self.batch_size, dtype=torch.int64, device=dev)
        loss_fn = torch.nn.MSELoss()

        def body():
            opt.zero_grad(set_to_none=False)
            loss = loss_fn(model(X.index_select(0, idx)), Y.index_select(0, idx))
            loss.backward()
            opt.step()

        g = _fit.capture_step(body, list(model.parameters()), opt, dev)
        st.update(graph=g, gkey=key, idx=idx)
        return st

    # ---- the reference API ------------------------------------------------------
    def _device_data(self, paths):
        dev = self._device_of()
        X = torch.from_numpy(self._features(paths).astype(np.float32)).to(dev)
        Y = torch.from_numpy(np.concatenate([p["returns"] for p in paths]).reshape(-1, 1).astype(np.float32)).to(dev)
        return X, Y

    def _sq_err(self, st, X, Y):
        with torch.no_grad():
            e = Y - st["model"](X)
            return e.pow(2).sum(), Y.pow(2).sum()

    def fit(self, paths, return_errors=False):
        """mlp_baseline.py:59-105 on the device."""
        if not torch.cuda.is_available():
            raise RuntimeError("mjrl_amd MLPBaseline fits on the GPU; no GPU is visible")
        st = self._to_device()
        X, Y = self._device_data(paths)
        return self._fit_device(st, X, Y, return_errors, comm=None)

    def fit_sharded(self, paths, comm, return_errors=False):
        """fit on the union of every rank's paths (one process per GPU)."""
        st = self._to_device()
        X, Y = self._device_data(paths)
        return self._fit_device(st, X, Y, return_errors, comm=comm)

    def _check_backend(self):
        if self.fit_backend not in FIT_BACKENDS:
            raise ValueError("MLPBaseline.fit_backend must be one of %s, not %r" % (FIT_BACKENDS, self.fit_backend))
        if self.fit_backend == "hip" and not 1 <= self.batch_size <= HIP_MAX_BATCH:
            raise ValueError('MLPBaseline.fit_backend = "hip" takes batch_size 1..%d, not %d'
                             % (HIP_MAX_BATCH, self.batch_size))

    def _fit_device(self, st, X, Y, return_errors, comm):
        if comm is None:
            self._check_backend()
        N_local = X.shape[0]
        dev = st["device"]
        if comm is not None and comm.world_size > 1:
            counts = torch.zeros(comm.world_size, dtype=torch.float64, device=_comm_dev(comm, dev))
            counts[comm.rank] = float(N_local)
            comm.allreduce_sum(counts)
            counts = counts.cpu().numpy().astype(np.int64)
            N = int(counts.sum())
            lo = int(counts[:comm.rank].sum())
        else:
            N, lo = N_local, 0
        if return_errors:
            e, y2 = self._sq_err(st, X, Y)
            error_before = self._ratio(e, y2, comm, dev)
        bs = self.batch_size
        for _ in range(self.epochs):
            # numpy's global RNG, as mlp_baseline.py:84 (rank 0 draws when sharded)
            if comm is not None and comm.world_size > 1:
                perm = torch.from_numpy(np.random.permutation(N) if comm.rank == 0 else np.zeros(N, np.int64))
                perm = perm.to(_comm_dev(comm, dev))
                comm.broadcast(perm)
                self._epoch_sharded(st, X, Y, perm.to(dev), lo, N_local, comm)
            else:
                rand_idx = torch.from_numpy(np.random.permutation(N)).to(dev)
                # fit_sharded stays on torch, on one rank too
                self._epoch(st, X, Y, rand_idx, backend="torch" if comm is not None else None)
        if return_errors:
            e, y2 = self._sq_err(st, X, Y)
            error_after = self._ratio(e, y2, comm, dev)
        self._from_device(st)
        if return_errors:
            return error_before, error_after

    @staticmethod
    def _ratio(e, y2, comm, dev):
        if comm is not None and comm.world_size > 1:
            t = torch.stack([e, y2]).double().to(_comm_dev(comm, dev))
            comm.allreduce_sum(t)
            e, y2 = t[0], t[1]
        return float(e.item() / (y2.item() + 1e-8))

    def _epoch(self, st, X, Y, rand_idx, backend=None):
        bs = self.batch_size
        nmb = int(X.shape[0] / bs) - 1
        if nmb <= 0:
            return
        if backend is None:
            self._check_backend()
            backend = self.fit_backend
        if backend == "hip":
            return self._epoch_hip(st, X, Y, rand_idx, nmb)
        try:
            st = self._step_graph(st, X, Y)
        except Exception:   # no graph capture available: eager steps, same math
            st["graph"] = None
        model, opt = st["model"], st["opt"]
        for mb in range(nmb):
            sel = rand_idx[mb * bs:(mb + 1) * bs]
            if st.get("graph") is not None:
                st["idx"].copy_(sel)
                st["graph"].replay()
            else:
                opt.zero_grad()
                loss = self.loss_function(model(X[sel]), Y[sel])
                loss.backward()
                opt.step()

    def _epoch_hip(self, st, X, Y, rand_idx, nmb):
        """The epoch's nmb steps as one mjrl_value_mlp_epoch call on the current
        stream: the device model's parameters and the device optimizer's moments
        are updated in place, then every step counter advances by nmb."""
        dev = st["device"]
        model, opt = st["model"], st["opt"]
        params = list(model.parameters())
        _fit.ensure_adam_state(opt, params, dev)   # a fresh optimizer has no state yet
        if X.dtype != torch.float32 or Y.dtype != torch.float32 or X.shape[1] != self.n + 4:
            raise ValueError("the fused value fit takes f32 features [T][n + 4] and f32 returns")
        X, Y, rand_idx = X.contiguous(), Y.contiguous(), rand_idx.contiguous()
        K = _lib.calls()
        st["hip_scratch"] = _fit.scratch(st.get("hip_scratch"), K.mjrl_value_mlp_scratch, (self.n, self.batch_size), dev)
        net = _fit.fill_net(_lib.ValueNet(), opt, params)
        hp = _fit.adam_hp(opt, params)
        with torch.cuda.device(dev):
            K.mjrl_value_mlp_epoch(X, Y, X.shape[0], self.n, rand_idx, nmb, self.batch_size, net, hp,
                                   st["hip_scratch"], None, None, _lib.stream_ptr(torch.cuda.current_stream(dev)))
        _fit.advance_steps(opt, params, nmb)

    def _epoch_sharded(self, st, X, Y, perm, lo, N_local, comm):
        """Data-parallel minibatches: this rank's members of each global minibatch
        contribute sum((yhat - y)^2) / bs to the gradient; the sum over ranks is
        the minibatch MSE gradient, then the same Adam step everywhere."""
        bs = self.batch_size
        model, opt = st["model"], st["opt"]
        params = list(model.parameters())
        nmb = int(perm.numel() / bs) - 1
        for mb in range(nmb):
            sel = perm[mb * bs:(mb + 1) * bs]
            mine = (sel >= lo) & (sel < lo + N_local)
            rows = (sel[mine] - lo)
            opt.zero_grad(set_to_none=False)
            if rows.numel():
                loss = ((model(X[rows]) - Y[rows]) ** 2).sum() / bs
                loss.backward()
            flat = torch.cat([p.grad.reshape(-1) for p in params])
            comm.allreduce_sum(flat)
            o = 0
            for p in params:
                k = p.numel()
                p.grad.copy_(flat[o:o + k].view_as(p))
                o += k
            opt.step()

    def predict_device(self, obs, path_off, lengths):
        """predict for every row of a staged batch at once: obs (device, [T][n]
        RL rows first), path_off (device i64 [P+1]), lengths (host [P]) -> f64
        device [T].  Features as _features (f64, then f32), one forward."""
        st = self._predict_state()
        feat = self.features_device(obs, path_off, lengths)
        with torch.no_grad():
            return st["model"](feat).to(torch.float64).reshape(-1)

    def features_device(self, obs, path_off, lengths):
        """_features(paths).astype('float32') (mlp_baseline.py:37-56, 108) of the
        staged rows, on obs's device: f32 [T][n + 4]."""
        dev = obs.device
        lengths = np.asarray(lengths, np.int64)
        T = int(np.sum(lengths))
        # float32(clip(x, +-10) / 10) with clip and division in f64 (np.clip(o) / 10.0
        # then .astype('float32')): bit for bit the reference's features when obs
        # holds the sampler's f64 values (BatchREINFORCE stages f64 for this baseline)
        o = (obs[:T].to(torch.float64).clamp(-10.0, 10.0) / 10.0).to(torch.float32)
        # the time features depend on the row's index in its path only: one f32
        # table from numpy's own al ** (j + 1) (torch's pow takes other roundings)
        tab = self.time_table(int(lengths.max()) if len(lengths) else 0, dev)
        start = torch.repeat_interleave(path_off[:-1], torch.from_numpy(lengths).to(dev))
        return torch.cat([o, tab[torch.arange(T, device=dev, dtype=torch.int64) - start]], 1)

    @staticmethod
    def time_table(H, dev):
        """The four time features of path indices 0 .. H - 1, f32 [H][4] on dev:
        numpy's own al ** (j + 1) (torch's pow takes other roundings)."""
        al = np.arange(int(H)) / 1000.0
        return torch.from_numpy(np.stack([al ** (j + 1) for j in range(4)], 1).astype(np.float32)).to(dev)

    def predict_features_device(self, feat):
        """predict_device's forward on a ready feature matrix (device f32
        [T][n + 4], features_device's bits: the streamed staging forms it while
        sampling, samplers/stream_staging.py) -> f64 device [T]."""
        st = self._predict_state()
        with torch.no_grad():
            return st["model"](feat).to(torch.float64).reshape(-1)

    def fit_features_device(self, feat, returns_dev, return_errors=False):
        """fit(paths) from the batch still in HBM: feat as predict_features_device
        takes it, returns_dev the paths' returns (device f64 [T]); the same
        minibatch draws from numpy's global RNG, the same steps."""
        st = self._to_device()
        Y = returns_dev.to(torch.float32).reshape(-1, 1)
        return self._fit_device(st, feat, Y, return_errors, comm=None)

    def predict(self, path):
        """mlp_baseline.py:107-115: one forward of the f32 features (on the GPU
        when one is visible, else on the CPU model)."""
        feat = self._features([path]).astype("float32")
        if torch.cuda.is_available():
            st = self._predict_state()
            with torch.no_grad():
                return st["model"](torch.from_numpy(feat).to(st["device"])).cpu().numpy().ravel()
        with torch.no_grad():
            return self.model(torch.from_numpy(feat)).numpy().ravel()


def _comm_dev(comm, dev):
    try:
        backend = comm.dist.get_backend(comm.group)
    except Exception:
        backend = "gloo"
    return dev if backend == "nccl" else torch.device("cpu")
