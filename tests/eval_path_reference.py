"""The evaluation forms of the block glue in float64 (a helper module like rowwise_passes_reference.py, not a conftest; CPU
only, nothing of se3conv3d_amd is imported): what `BatchNormPC`, `SkipConnection` and the three blocks compute under
`eval()`, restated per element, with the scale each element is held against, and a float32 emulation of the two row-wise
formulas from which the bounds are taken (8 x the emulation's own largest error / scale, the factor of
pne_reference.py::bounds).

    eval batch norm   y = (x - running_mean) / sqrt(running_var + eps) * weight + bias         scale |x - rm| |w| / sigma + |b|
    eval skip         out = x * gamma + y   for any drop_prob (no draw, no 1 / keep)            scale |x gamma| + |y|
    blocks            ResNetFormer, ResNetB, ResConvNeXt composed of these, the group norm of group_norm_reference.py
                      (`two_pass_fp64`; it has no eval form), float64 linear layers, the erf GELU in float64, and the
                      convolution of oracle/se3conv_oracle.py fed float64 tensors

`train=True` switches batch norm to batch statistics (biased variance under the root) and returns the running statistics
after the reference's update (momentum 0.2, unbiased variance): in that form the restatement is pinned to the reference's
own Python (tests/golden/*_block.npz) before anybody trusts its eval form.

`fault=` plants one of FAULTS, the mix-ups an evaluation path can make silently:
    batch_stats        eval batch norm normalises with the batch's own statistics
    biased_running_var the running variance is updated with the biased variance (shows in the statistics a training step
                       leaves, hence in every later eval)
    no_eps             eps dropped under the root
    keep_factor        the 1 / keep drop-path factor applied in eval
    no_gamma           gamma dropped from the skip
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import se3conv_oracle as O  # noqa: E402

from group_norm_reference import two_pass_fp64  # noqa: E402

D, F = np.float64, np.float32
EPS = 1e-5          # torch.nn.BatchNorm1d's default, what BatchNormPC builds
MOMENTUM = 0.2      # layers/BatchNormPC.py
FAULTS = ("batch_stats", "biased_running_var", "no_eps", "keep_factor", "no_gamma")
BN_FAULTS = FAULTS[:3]
BLOCKS = ("ResNetFormer", "ResNetB", "ResConvNeXt")


def _w(a, T=D):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).astype(T)


# ------------------------------------------------------------------------------------------------ row-wise pieces
def batch_stats(x):
    """(mean, biased variance, unbiased variance) per channel in float64, the variance from the centred values."""
    x = _w(x)
    n = x.shape[0]
    mu = x.mean(0)
    var = ((x - mu) ** 2).mean(0)
    return mu, var, var * n / (n - 1.0) if n > 1 else var


def batch_norm(x, weight, bias, running_mean, running_var, eps=EPS, train=False, momentum=MOMENTUM, fault=None, T=D):
    """`(y, scale, new_running_mean, new_running_var)`.  eval: the formula of the module docstring on the running statistics,
    which come back unchanged.  `train=True`: batch statistics and the updated running statistics.  T = float32: the
    emulation of the eval formula, every step one float32 numpy operation."""
    x64, w, b = _w(x), _w(weight, T).reshape(-1), _w(bias, T).reshape(-1)
    rm, rv = _w(running_mean, T).reshape(-1), _w(running_var, T).reshape(-1)
    e = T(0.0) if fault == "no_eps" else T(F(eps))
    if train or fault == "batch_stats":
        mu, var, unbiased = batch_stats(x64)
        mean, under = mu.astype(T), var.astype(T)
    else:
        mean, under = rm, rv
    sigma = np.sqrt(under + e)
    y = (_w(x, T) - mean) / sigma * w + b
    scale = np.abs(x64 - _w(mean)) * np.abs(_w(w)) / _w(sigma) + np.abs(_w(b))
    if train:
        new_var = var if fault == "biased_running_var" else unbiased
        rm = (1.0 - momentum) * _w(rm) + momentum * mu
        rv = (1.0 - momentum) * _w(rv) + momentum * new_var
    return y, scale, rm, rv


def skip(x, y, gamma, drop_prob=0.0, fault=None, T=D):
    """`(out, scale)` of the eval skip connection: `x * gamma + y` whatever `drop_prob` is."""
    g = np.ones((1, np.asarray(_w(x)).shape[1]), T) if fault == "no_gamma" else _w(gamma, T).reshape(1, -1)
    f = T(1.0 / (1.0 - drop_prob)) if fault == "keep_factor" else T(1.0)
    out = _w(x, T) * g * f + _w(y, T)
    return out, np.abs(_w(x) * _w(g) * D(f)) + np.abs(_w(y))


def bn_bounds_case(rows, c, seed):
    """Input with a per-channel offset and scale, non-trivial weight, bias and running statistics: what the bound of the
    eval batch norm is measured on and what the GPU test feeds the module."""
    g = np.random.default_rng(seed)
    x = (g.standard_normal((rows, c)) * 10.0 ** g.uniform(-1, 1, c) + g.uniform(-3, 3, c)).astype(F)
    return {"x": x, "weight": g.uniform(0.5, 1.5, c).astype(F) * g.choice([-1.0, 1.0], c).astype(F),
            "bias": g.uniform(-1, 1, c).astype(F), "running_mean": g.uniform(-3, 3, c).astype(F),
            "running_var": (10.0 ** g.uniform(-2, 2, c)).astype(F)}


def skip_bounds_case(rows, c, seed):
    g = np.random.default_rng(seed)
    return {"x": g.standard_normal((rows, c)).astype(F), "y": g.standard_normal((rows, c)).astype(F),
            "gamma": (g.uniform(0.1, 2.0, (1, c)) * g.choice([-1.0, 1.0], (1, c))).astype(F)}


BOUND_ROWS, BOUND_CHANNELS = (1, 255, 256, 257), (8, 24, 64)


def worst(got, ref, scale):
    got, ref, scale = _w(got), _w(ref), _w(scale)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    return float(ratio.max()) if ratio.size else 0.0


def emulated_max():
    """{"bn_eval": r, "skip_eval": r}: the largest error / scale of the float32 emulation over the shapes of the GPU test."""
    out = {"bn_eval": 0.0, "skip_eval": 0.0}
    for rows in BOUND_ROWS:
        for c in BOUND_CHANNELS:
            d = bn_bounds_case(rows, c, 1000 * rows + c)
            ref, scale, _, _ = batch_norm(**d)
            out["bn_eval"] = max(out["bn_eval"], worst(batch_norm(**d, T=F)[0], ref, scale))
            s = skip_bounds_case(rows, c, 2000 * rows + c)
            ref, scale = skip(**s)
            out["skip_eval"] = max(out["skip_eval"], worst(skip(**s, T=F)[0], ref, scale))
    return out


def bounds():
    return {k: 8.0 * v for k, v in emulated_max().items()}


# ------------------------------------------------------------------------------------------------ dense pieces
def gelu(x):
    x = torch.as_tensor(_w(x))
    return (0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))).numpy()


def linear(x, weight, bias):
    return _w(x) @ _w(weight).T + _w(bias).reshape(1, -1)


class Geometry:
    """The cloud of a block fixture as the oracle takes it: float64 points and frames, the oracle's own ball query (on the
    float32 points, as the fixture's generator ran it)."""

    def __init__(self, pts, frames, batch, radius):
        t = lambda v: torch.as_tensor(np.asarray(v))
        self.batch = np.asarray(batch)
        self.n_batches = int(self.batch.max()) + 1
        self.neighbors, _ = O.ball_query(t(pts), t(pts), t(batch), t(batch), float(radius))
        self.pts, self.frames = t(pts).double(), t(frames).double()

    def conv(self, x, state, prefix="spatial_conv_."):
        t = lambda k: torch.as_tensor(_w(state[prefix + k]))
        out = O.conv_forward(self.pts, self.pts, self.frames, self.frames, self.neighbors, torch.as_tensor(_w(x)),
                             t("proj_axes_"), t("proj_biases_"), t("conv_weights_"), t("norm_neigh_dist_"), t("norm_num_neighs_"))
        assert out.dtype == torch.float64
        return out.numpy()


class _Norms:
    """The norm layers of one block forward: 'batch' (state keys `<name>.layer_.*`) or 'group' (`<name>.gamma_`, `.betas_`)."""

    def __init__(self, kind, state, geom, train, fault, groups=8):
        self.kind, self.state, self.geom, self.train, self.fault, self.groups = kind, state, geom, train, fault, groups
        self.after, self.inputs = {}, {}

    def __call__(self, name, x):
        s = self.state
        self.inputs[name] = batch_stats(x)
        if self.kind == "group":
            frames = x.shape[0] // self.geom.batch.shape[0]
            assert frames == 1, "two_pass_fp64 restates the reference's group norm, which never ran with frames"
            return two_pass_fp64(x, s[name + ".gamma_"], s[name + ".betas_"], self.geom.batch, self.geom.n_batches, self.groups,
                                 np.zeros_like(x))[0]
        p = name + ".layer_."
        fault = self.fault if self.fault in BN_FAULTS else None
        y, _, rm, rv = batch_norm(x, s[p + "weight"], s[p + "bias"], s[p + "running_mean"], s[p + "running_var"],
                                  train=self.train, fault=fault)
        self.after[p + "running_mean"], self.after[p + "running_var"] = rm, rv
        return y


def block_forward(cls, state, geom, x, norm="batch", train=False, drop_prob=0.0, fault=None, norm_inputs=None):
    """`(out, after)`: the forward of block `cls` (a name of BLOCKS) with the reference's state_dict keys, in float64;
    `after`: the running statistics of its batch norms behind the call (those of `state` in eval).  In `train` form the drop
    path is the identity only for `drop_prob == 0`, the one the fixtures were recorded with.  `norm_inputs` (a dict): receives
    the batch statistics `(mean, biased variance, unbiased variance)` of every norm layer's input."""
    assert cls in BLOCKS and not (train and drop_prob != 0.0)
    norms = _Norms(norm, state, geom, train, fault)
    if norm_inputs is not None:
        norms.inputs = norm_inputs
    sfault = fault if fault in ("keep_factor", "no_gamma") else None
    sk = lambda name, a, b: skip(a, b, state[name + ".gamma_"], drop_prob, sfault)[0]
    lin = lambda name, v: linear(v, state[name + ".weight"], state[name + ".bias"])
    x = _w(x)
    same = state["linear_2_.weight"].shape[0] == x.shape[1]
    if cls == "ResNetFormer":
        h = sk("skip_path_1_", geom.conv(norms("norm_1_", x), state), x)
        y = lin("linear_2_", gelu(lin("linear_1_", norms("norm_2_", h))))
        return sk("skip_path_2_", y, h if same else lin("skip_conv_", h)), norms.after
    if cls == "ResNetB":
        h = geom.conv(lin("linear_1_", norms("norm_", x)), state)
        y = lin("linear_2_", gelu(h))
    else:
        y = lin("linear_2_", gelu(lin("linear_1_", norms("norm_", geom.conv(x, state)))))
    return sk("skip_path_", y, x if same else lin("skip_conv_", x)), norms.after


def rel_err(a, b):
    a, b = _w(a), _w(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def fixture(name):
    """`(cls, state, geometry, d)` of tests/golden/<name>_block.npz."""
    d = np.load(os.path.join(ROOT, "tests", "golden", f"{name}_block.npz"))
    state = {k[len("state/"):]: np.asarray(d[k]) for k in d.files if k.startswith("state/")}
    cls = {"resnetformer": "ResNetFormer", "resnetb": "ResNetB", "resconvnext": "ResConvNeXt"}[name]
    return cls, state, Geometry(d["pts"], d["frames"], d["batch"], d["radius"]), d


def with_batch_norm(state, seed):
    """The state of a ResNetB / ResConvNeXt fixture with `BatchNormPC` in place of its group norm: the group norm's two
    parameters replaced by seeded batch-norm weights and running statistics (no fixture of the reference holds these blocks
    with a batch norm; its pieces are pinned on the ResNetFormer fixture)."""
    c = state["norm_.gamma_"].shape[1]
    g = np.random.default_rng(seed)
    out = {k: v for k, v in state.items() if not k.startswith("norm_.")}
    out.update({"norm_.layer_.weight": g.uniform(0.5, 1.5, c).astype(F), "norm_.layer_.bias": g.uniform(-0.5, 0.5, c).astype(F),
                "norm_.layer_.running_mean": g.uniform(-0.5, 0.5, c).astype(F),
                "norm_.layer_.running_var": g.uniform(0.3, 3.0, c).astype(F),
                "norm_.layer_.num_batches_tracked": np.asarray(1, np.int64)})
    return out


def evaluated_state(state, d):
    """The ResNetFormer fixture's state with the running statistics a training step left (`after/`): what `eval()` reads."""
    out = dict(state)
    for k in d.files:
        if k.startswith("after/"):
            out[k[len("after/"):]] = np.asarray(d[k])
    return out


def drawn_state(cls, state, geom, x, seed):
    """`state` (batch-norm form) with running statistics from a seeded generator, drawn against the batch statistics of each
    norm layer's input: mean = batch mean + U(-1, 1) batch sigma, variance = batch variance x 10^U(-3, 0).  Far from the batch
    statistics in every channel, and small enough that a dropped eps (1e-5 under the root) and a biased update (1 / n of
    the batch variance) move the output by more than the bounds the GPU test holds it to -- which they do not with the
    statistics of the ResNetFormer fixture's `after/` entries, whose variances sit near 1."""
    inputs = {}
    block_forward(cls, state, geom, x, norm="batch", train=True, norm_inputs=inputs)
    g = np.random.default_rng(seed)
    out = dict(state)
    for name in sorted(inputs):
        mu, var, _ = inputs[name]
        out[name + ".layer_.running_mean"] = (mu + g.uniform(-1, 1, mu.shape) * np.sqrt(var)).astype(F)
        out[name + ".layer_.running_var"] = (var * 10.0 ** g.uniform(-3, 0, mu.shape)).astype(F)
    return out


def eval_states(name):
    """`(cls, geometry, d, [(label, norm kind, state)])`: the states the CPU fault test and the GPU block test both use.
    ResNetFormer: the fixture's state with its `after/` statistics, and with drawn ones.  ResNetB / ResConvNeXt: the
    fixture's own (group norm), and a batch-norm form with drawn statistics."""
    cls, state, geom, d = fixture(name)
    if cls == "ResNetFormer":
        return cls, geom, d, [("after", "batch", evaluated_state(state, d)), ("drawn", "batch", drawn_state(cls, state, geom, d["x"], 11))]
    return cls, geom, d, [("group", "group", state), ("drawn", "batch", drawn_state(cls, with_batch_norm(state, 7), geom, d["x"], 11))]


def after_training_step(cls, state, geom, x, fault=None):
    """`state` with the running statistics one training-form forward leaves (a planted `biased_running_var` included)."""
    return {**state, **block_forward(cls, state, geom, x, norm="batch", train=True, fault=fault)[1]}
