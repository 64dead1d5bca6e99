"""The reference's parameter network ``ddr.nn.kan`` (``src/ddr/nn/kan.py:11-62``) without pykan.

``Linear(F, H)`` -> ``num_hidden_layers`` pykan ``KAN([H, H])`` layers -> ``Linear(H, O)`` -> sigmoid; the output
is a dict ``name -> (N,)`` in [0, 1] (the routing engine denormalises, as in the reference).  A KAN layer
restates pykan 0.2.x (``MultKAN`` with width ``[H, H]``, no multiplication nodes, symbolic branch off)::

    B^0_j(x) = [t_j <= x < t_{j+1}]
    B^k_j(x) = (x - t_j) / (t_{j+k} - t_j) B^{k-1}_j(x) + (t_{j+k+1} - x) / (t_{j+k+1} - t_{j+1}) B^{k-1}_{j+1}(x)
    y_o = sum_i mask[i,o] (scale_base[i,o] silu(h_i) + scale_sp[i,o] sum_j coef[i,o,j] B^k_j(h_i))
    y   = node_scale (subnode_scale y + subnode_bias) + node_bias

* :class:`kan` -- the reference's constructor and call, forward and backward as HIP launches
  (``ddr_kan_forward_f32`` / ``ddr_kan_backward_f32``, ``csrc/kan.hip``): L launches forward, L + 4 backward,
  bitwise reproducible.  HIP device and fp32 only; there is no fallback.
* :class:`TorchKan` -- the same function and parameters in PyTorch ops (pykan's form: it materialises the
  (N, H, G + k) basis tensor), for any device and dtype.  In fp64 on the CPU it is the numerical model of the
  tests; in fp32 on the GPU it is the launch-count and time baseline.
* :func:`load_checkpoint` -- the reference's helper (``scripts_utils.py:45-73``).

**Parameters.**  The trainable values are ONE flat fp32 ``Parameter`` ``flat`` (so ``ClipAdam``, the clipping
norm and the gradient all-reduce touch one buffer)::

    input.weight (H, F) | input.bias (H) |
    per layer l: coef (H, H, G + k) [in, out, j] | scale_base (H, H) [in, out] | scale_sp (H, H) |
    output.weight (O, H) | output.bias (O)

and the tensors the reference does not train are ONE flat buffer ``consts``::

    per layer l: grid (H, G + 1 + 2k) | mask (H, H) [in, out] | node_scale (H) | node_bias (H) |
                 subnode_scale (H) | subnode_bias (H)

``views()`` / ``const_views()`` give the named tensors (views of the two vectors, under the reference's
state-dict keys).  ``state_dict()`` emits and ``load_state_dict()`` accepts exactly the reference's keys and
shapes (``layers.{l}.act_fun.0.coef`` ...; the symbolic tensors are emitted as zeros, and a non-zero symbolic
mask is refused), so the reference's checkpoints load here and a checkpoint saved here loads in DDR.

**What is pinned.**  pykan cannot run where this was written, so parity with pykan itself is NOT pinned: what is
pinned is the key/shape contract of both published checkpoints and the spline identities (partition of unity,
Greville abscissae, zero outside the knots) of ``tests/test_kan_api.py``.  The initialisation follows pykan's
published scheme (uniform grid on [-1, 1] extended by k steps each side, ``scale_base ~ U(-1, 1) / sqrt(in)``,
``scale_sp = 1 / sqrt(in)``, ``coef`` a least-squares fit of ``U(-0.5, 0.5) 0.3 / G`` noise at the grid points,
Kaiming / Xavier(0.1) for the two Linears as ``kan.py:45-48``); bit-parity with a seeded pykan initialisation is
not claimed.
"""

from __future__ import annotations

import ctypes as C
import math
from pathlib import Path

import torch

from .. import _lib

# the supported envelope of the HIP path (csrc/kan.h)
MAX_F, MAX_H, MAX_O, MAX_L, MAX_K, MAX_TABLE = 32, 32, 8, 4, 3, 32768


def check_envelope(F: int, H: int, O: int, L: int, G: int, k: int) -> None:
    """ValueError for an architecture ``csrc/kan.hip`` does not take (the limits of ``kan_validate``)."""
    for name, v, lo, hi in (("input features", F, 1, MAX_F), ("hidden_size", H, 1, MAX_H),
                            ("learnable parameters", O, 1, MAX_O), ("num_hidden_layers", L, 1, MAX_L), ("k", k, 1, MAX_K)):
        if not lo <= v <= hi:
            raise ValueError(f"the fused KAN takes {lo} <= {name} <= {hi} (got {v})")
    if G < 1:
        raise ValueError(f"the fused KAN takes grid >= 1 (got {G})")
    if H * H * (G + k) > MAX_TABLE:
        raise ValueError(f"the fused KAN takes hidden_size^2 (grid + k) <= {MAX_TABLE} (got {H * H * (G + k)})")


def _trainable_shapes(F, H, O, L, G, k):
    s = [("input.weight", (H, F)), ("input.bias", (H,))]
    for l in range(L):
        p = f"layers.{l}.act_fun.0."
        s += [(p + "coef", (H, H, G + k)), (p + "scale_base", (H, H)), (p + "scale_sp", (H, H))]
    return s + [("output.weight", (O, H)), ("output.bias", (O,))]


def _const_shapes(F, H, O, L, G, k):
    s = []
    for l in range(L):
        p = f"layers.{l}."
        s += [(p + "act_fun.0.grid", (H, G + 1 + 2 * k)), (p + "act_fun.0.mask", (H, H)), (p + "node_scale_0", (H,)),
              (p + "node_bias_0", (H,)), (p + "subnode_scale_0", (H,)), (p + "subnode_bias_0", (H,))]
    return s


def _split(vec: torch.Tensor, shapes) -> dict[str, torch.Tensor]:
    out, o = {}, 0
    for name, shp in shapes:
        n = math.prod(shp)
        out[name] = vec[o:o + n].view(shp)
        o += n
    return out


def _count(shapes) -> int:
    return sum(math.prod(shp) for _, shp in shapes)


def b_batch(x: torch.Tensor, grid: torch.Tensor, k: int) -> torch.Tensor:
    """Every B-spline basis of order k: x (N, H), grid (H, G + 1 + 2k) -> (N, H, G + k) (pykan's ``B_batch``)."""
    xe = x.unsqueeze(2)
    g = grid.unsqueeze(0)
    if k == 0:
        value = ((xe >= g[:, :, :-1]) & (xe < g[:, :, 1:])).to(x.dtype)
    else:
        b = b_batch(x, grid, k - 1)
        value = ((xe - g[:, :, :-(k + 1)]) / (g[:, :, k:-1] - g[:, :, :-(k + 1)]) * b[:, :, :-1]
                 + (g[:, :, k + 1:] - xe) / (g[:, :, k + 1:] - g[:, :, 1:-k]) * b[:, :, 1:])
    return torch.nan_to_num(value)


def _check_knots(grid: torch.Tensor, what: str) -> None:
    if not bool((grid[:, 1:] > grid[:, :-1]).all()):
        raise ValueError(f"{what}: every knot row must be strictly increasing")


class _KanBase(torch.nn.Module):
    def __init__(self, input_var_names, learnable_parameters, hidden_size, num_hidden_layers, grid, k, seed,
                 device="cpu"):
        super().__init__()
        self.input_size = len(input_var_names)
        self.hidden_size = int(hidden_size)
        self.learnable_parameters = list(learnable_parameters)
        self.output_size = len(self.learnable_parameters)
        self.num_hidden_layers = int(num_hidden_layers)
        self.grid_size, self.k = int(grid), int(k)
        if min(self.input_size, self.hidden_size, self.output_size, self.num_hidden_layers, self.grid_size, self.k) < 1:
            raise ValueError("a KAN needs at least one input, hidden unit, output, layer, grid interval and k >= 1")
        self._check_architecture()
        flat = torch.zeros(_count(_trainable_shapes(*self.arch)))
        consts = torch.zeros(_count(_const_shapes(*self.arch)))
        self._init(flat, consts, int(seed))
        self.flat = torch.nn.Parameter(flat.to(device))
        self.register_buffer("consts", consts.to(device), persistent=False)

    def _check_architecture(self) -> None:
        pass

    @property
    def arch(self):
        """(F, H, O, L, G, k)"""
        return (self.input_size, self.hidden_size, self.output_size, self.num_hidden_layers, self.grid_size, self.k)

    def views(self, flat: torch.Tensor | None = None) -> dict[str, torch.Tensor]:
        """The trainable tensors under the reference's keys, as views of ``flat`` (default: ``self.flat``; pass
        ``self.flat.grad`` for the gradients)."""
        return _split(self.flat if flat is None else flat, _trainable_shapes(*self.arch))

    def const_views(self) -> dict[str, torch.Tensor]:
        """The non-trainable tensors (grid, mask, node / subnode scale and bias) as views of ``consts``."""
        return _split(self.consts, _const_shapes(*self.arch))

    def _init(self, flat, consts, seed):
        F, H, O, L, G, k = self.arch
        gen = torch.Generator().manual_seed(seed)
        v, c = _split(flat, _trainable_shapes(*self.arch)), _split(consts, _const_shapes(*self.arch))
        v["input.weight"].copy_(torch.randn(H, F, generator=gen) * math.sqrt(2.0 / F))
        v["output.weight"].copy_(torch.randn(O, H, generator=gen) * (0.1 * math.sqrt(2.0 / (H + O))))
        knots = torch.linspace(-1, 1, G + 1)[None, :].expand(H, G + 1)
        step = (knots[:, [-1]] - knots[:, [0]]) / G
        for _ in range(k):
            knots = torch.cat([knots[:, [0]] - step, knots, knots[:, [-1]] + step], dim=1)
        for l in range(L):
            p = f"layers.{l}."
            c[p + "act_fun.0.grid"].copy_(knots)
            c[p + "act_fun.0.mask"].fill_(1.0)
            c[p + "node_scale_0"].fill_(1.0)
            c[p + "subnode_scale_0"].fill_(1.0)
            v[p + "act_fun.0.scale_base"].copy_((torch.rand(H, H, generator=gen) * 2 - 1) / math.sqrt(H))
            v[p + "act_fun.0.scale_sp"].fill_(1.0 / math.sqrt(H))
            # coef: the least-squares fit of noise (G + 1, in, out) at the grid points (pykan's curve2coef)
            noise = ((torch.rand(G + 1, H, H, generator=gen) - 0.5) * 0.3 / G).double()
            basis = b_batch(knots[:, k:G + k + 1].t().double(), knots.double(), k)  # (G + 1, in, G + k)
            coef = torch.linalg.lstsq(basis.permute(1, 0, 2), noise.permute(1, 0, 2)).solution  # (in, G + k, out)
            v[p + "act_fun.0.coef"].copy_(coef.permute(0, 2, 1))

    # the reference's state dict: its keys, shapes and order
    def _reference_items(self):
        v, c = self.views(), self.const_views()
        H = self.hidden_size
        items = [("input.weight", v["input.weight"]), ("input.bias", v["input.bias"])]
        for l in range(self.num_hidden_layers):
            p = f"layers.{l}."
            items += [(p + n, c[p + n]) for n in ("node_bias_0", "node_scale_0", "subnode_bias_0", "subnode_scale_0")]
            items += [(p + "act_fun.0.grid", c[p + "act_fun.0.grid"]), (p + "act_fun.0.coef", v[p + "act_fun.0.coef"]),
                      (p + "act_fun.0.mask", c[p + "act_fun.0.mask"]),
                      (p + "act_fun.0.scale_base", v[p + "act_fun.0.scale_base"]),
                      (p + "act_fun.0.scale_sp", v[p + "act_fun.0.scale_sp"]),
                      (p + "symbolic_fun.0.mask", (H, H)), (p + "symbolic_fun.0.affine", (H, H, 4))]
        return items + [("output.weight", v["output.weight"]), ("output.bias", v["output.bias"])]

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for key, t in self._reference_items():
            if isinstance(t, tuple):  # the symbolic branch is off: zeros
                t = torch.zeros(t, dtype=self.flat.dtype, device=self.flat.device)
            destination[prefix + key] = t if keep_vars else t.detach()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        items = self._reference_items()
        known = {prefix + key for key, _ in items}
        if strict:
            unexpected_keys += [k for k in state_dict if k.startswith(prefix) and k not in known]
        todo, ok = [], True
        for key, t in items:
            src = state_dict.get(prefix + key)
            if src is None:
                missing_keys.append(prefix + key)
                continue
            shape = t if isinstance(t, tuple) else tuple(t.shape)
            if tuple(src.shape) != shape:
                error_msgs.append(f"size mismatch for {prefix + key}: checkpoint {tuple(src.shape)}, model {shape}")
                ok = False
            elif key.endswith("symbolic_fun.0.mask"):
                if bool((src != 0).any()):
                    error_msgs.append(f"{prefix + key} has non-zero entries: symbolic activations are not implemented")
                    ok = False
            elif key.endswith("act_fun.0.grid") and not bool((src[:, 1:] > src[:, :-1]).all()):
                error_msgs.append(f"{prefix + key}: every knot row must be strictly increasing")
                ok = False
            elif not isinstance(t, tuple):
                todo.append((t, src))
        if ok:
            with torch.no_grad():
                for t, src in todo:
                    t.copy_(src)

    def _validate_knots(self) -> None:
        """ValueError unless every knot row is strictly increasing; checked again only after ``consts`` changed
        (the check reads the knots back from the device)."""
        tag = (self.consts.data_ptr(), self.consts._version)
        if getattr(self, "_knots_checked", None) != tag:
            for name, t in self.const_views().items():
                if name.endswith("act_fun.0.grid"):
                    _check_knots(t, name)
            self._knots_checked = tag

    def forward(self, *args, **kwargs) -> dict[str, torch.Tensor]:
        u = self._u(kwargs["inputs"])
        ut = u.transpose(0, 1)
        return {key: ut[idx] for idx, key in enumerate(self.learnable_parameters)}


class TorchKan(_KanBase):
    """The network in PyTorch ops, pykan's form; any device and dtype (``.double()`` for the fp64 model)."""

    def _u(self, x: torch.Tensor) -> torch.Tensor:
        v, c = self.views(), self.const_views()
        self._validate_knots()
        h =torch.nn.functional.linear(x.to(self.flat.dtype), v["input.weight"], v["input.bias"])
        for l in range(self.num_hidden_layers):
            p = f"layers.{l}."
            a = p + "act_fun.0."
            spline = torch.einsum("nij,ioj->nio", b_batch(h, c[a + "grid"], self.k), v[a + "coef"])
            y = v[a + "scale_base"][None] * torch.nn.functional.silu(h)[:, :, None] + v[a + "scale_sp"][None] * spline
            y = (c[a + "mask"][None] * y).sum(dim=1)
            y = c[p + "subnode_scale_0"][None] * y + c[p + "subnode_bias_0"][None]
            h = c[p + "node_scale_0"][None] * y + c[p + "node_bias_0"][None]
        return torch.sigmoid(torch.nn.functional.linear(h, v["output.weight"], v["output.bias"]))


def _check_device_f32(t: torch.Tensor, dev: torch.device, what: str, shape) -> None:
    """The C ABI takes raw device pointers: a host, fp64, strided or other-device tensor would be read as fp32
    device memory (a GPU memory fault, not a Python error), so reject it here (as ``pnet._check_device_f32``)."""
    if not (t.is_cuda and t.device == dev):
        raise ValueError(f"the fused KAN's {what} must be on {dev} (got {t.device})")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"the fused KAN's {what} must be contiguous float32")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"the fused KAN's {what} must have shape {tuple(shape)}, got {tuple(t.shape)}")


class _KanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, flat, consts, arch, save):
        lib = _lib.load()
        F, H, O, L, G, k = arch
        desc = _lib.KanDesc(F, H, O, L, G, k)
        N, dev = x.shape[0], x.device
        u = torch.empty((N, O), device=dev, dtype=torch.float32)
        h = torch.empty((L + 1, N, H), device=dev, dtype=torch.float32) if save else None
        work = None
        if not save and L > 1:
            work = torch.empty(int(lib.ddr_kan_work_bytes(C.byref(desc), N, 0)), device=dev, dtype=torch.uint8)
        _lib.check(lib.ddr_kan_forward_f32(C.byref(desc), N, x.data_ptr(), flat.data_ptr(), consts.data_ptr(),
                                           _lib.ptr(h), u.data_ptr(), _lib.ptr(work), _lib.stream_ptr(dev)))
        if save:
            ctx.save_for_backward(x, flat, consts, h, u)
            ctx.arch = arch
        return u

    @staticmethod
    def backward(ctx, gu):
        x, flat, consts, h, u = ctx.saved_tensors
        lib = _lib.load()
        desc = _lib.KanDesc(*ctx.arch)
        N, dev = x.shape[0], x.device
        gu = gu.to(torch.float32).contiguous()
        _check_device_f32(gu, dev, "output gradient", u.shape)
        grad = torch.empty_like(flat)
        work = torch.empty(int(lib.ddr_kan_work_bytes(C.byref(desc), N, 1)), device=dev, dtype=torch.uint8)
        _lib.check(lib.ddr_kan_backward_f32(C.byref(desc), N, x.data_ptr(), flat.data_ptr(), consts.data_ptr(),
                                            h.data_ptr(), u.data_ptr(), gu.data_ptr(), grad.data_ptr(),
                                            work.data_ptr(), _lib.stream_ptr(dev)))
        return None, grad, None, None, None


class kan(_KanBase):
    """``ddr.nn.kan`` (``kan.py:11-62``: the same constructor, ``forward(inputs=...) -> dict``), forward and
    backward in HIP.  The module must be on the HIP device in fp32; the attributes get no gradient."""

    def _check_architecture(self) -> None:
        check_envelope(*self.arch)

    def _u(self, x: torch.Tensor) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError("the fused KAN runs on the HIP device only: inputs must be a device tensor (no CPU fallback)")
        if x.dim() != 2 or x.shape[1] != self.input_size or x.shape[0] < 1:
            raise ValueError(f"inputs must be (N >= 1, {self.input_size})")
        grad = torch.is_grad_enabled()
        if grad and x.requires_grad:
            raise ValueError("the fused KAN produces no gradient of its inputs: detach them (or use TorchKan)")
        x = x.detach().to(torch.float32).contiguous()
        # the vectors as the kernels read them: fp32, contiguous, on x's device (not after .double() or
        # without .to(device))
        _check_device_f32(self.flat, x.device, "parameters", (_count(_trainable_shapes(*self.arch)),))
        _check_device_f32(self.consts, x.device, "constants", (_count(_const_shapes(*self.arch)),))
        self._validate_knots()
        return _KanFn.apply(x, self.flat, self.consts, self.arch, grad and self.flat.requires_grad)


def load_checkpoint(model: torch.nn.Module, checkpoint_path, device) -> dict:
    """Load a DDR checkpoint and apply its ``model_state_dict`` to ``model``; returns the whole checkpoint (epoch,
    mini_batch, optimizer state ...), as the reference's ``load_checkpoint`` (``scripts_utils.py:45-73``)."""
    state = torch.load(Path(checkpoint_path), map_location=device, weights_only=False)
    state_dict = state["model_state_dict"]
    for key in state_dict.keys():
        state_dict[key] = state_dict[key].to(device)
    model.load_state_dict(state_dict)
    return state
