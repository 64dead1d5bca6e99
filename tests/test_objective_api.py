"""ddr_amd.train.daily_objective without a GPU: the Python argument checks, the C ABI's refusals before any launch,
and the binding against the header."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from ddr_amd import _lib
from ddr_amd.train import OBJECTIVE_KINDS, ObjectiveTerms, daily_objective

HEADER = Path(__file__).resolve().parents[1] / "include" / "ddr_mc.h"
FUNCTIONS = ("ddr_daily_objective_f32", "ddr_daily_objective_work_bytes")
CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "float": C.c_float}


def header_code() -> str:
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def test_cpu_tensors_raise():
    z = torch.zeros
    with pytest.raises(RuntimeError, match="HIP device only"):
        daily_objective(z(2, 3), z(2, 3), 0)
    for kind in OBJECTIVE_KINDS:
        with pytest.raises(RuntimeError, match="HIP device only"):
            daily_objective(z(2, 3), z(2, 3), 1, kind, drop=z(2, dtype=torch.bool), weight=z(2), eps=0.5, count=3.0,
                            terms=True)


def test_argument_errors():
    """Shape, dtype, kind, warm-up, eps and count are checked before the device, so they raise for host tensors."""
    z = torch.zeros
    with pytest.raises(ValueError, match="float32"):
        daily_objective(z(2, 3, dtype=torch.float64), z(2, 3), 0)
    with pytest.raises(ValueError, match="float32"):
        daily_objective(z(2, 3), z(2, 3, dtype=torch.float16), 0)
    for a, b in ((z(2, 3), z(2, 4)), (z(2, 3), z(3)), (z(3), z(3)), (z(2, 3, 4), z(2, 3, 4))):
        with pytest.raises(ValueError, match="same"):
            daily_objective(a, b, 0)
    for warmup in (-1, 3, 7, 1.5):
        with pytest.raises(ValueError, match="warmup"):
            daily_objective(z(2, 3), z(2, 3), warmup)
    for kind in ("L1", "mae", "", None, 0):
        with pytest.raises(ValueError, match="kind"):
            daily_objective(z(2, 3), z(2, 3), 0, kind)
    for eps in (-1e-9, float("nan")):
        with pytest.raises(ValueError, match="eps"):
            daily_objective(z(2, 3), z(2, 3), 0, "nse", eps=eps)
    for drop in (z(2), z(3, dtype=torch.bool), z(2, 1, dtype=torch.bool)):
        with pytest.raises(ValueError, match="drop"):
            daily_objective(z(2, 3), z(2, 3), 0, drop=drop)
    for weight in (z(2, dtype=torch.float64), z(3), z(2, 1)):
        with pytest.raises(ValueError, match="weight"):
            daily_objective(z(2, 3), z(2, 3), 0, weight=weight)
    for count in (0.0, -2.0, float("nan"), z(2), z((), dtype=torch.float64)):
        with pytest.raises(ValueError, match="count"):
            daily_objective(z(2, 3), z(2, 3), 0, count=count)
    with pytest.raises(ValueError, match="8192"):
        daily_objective(z(1, 8193), z(1, 8193), 0)
    with pytest.raises(TypeError):
        daily_objective(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32), 0)
    assert [f.name for f in ObjectiveTerms.__dataclass_fields__.values()] == ["term", "days", "used"]


def call(lib, kind=0, G=2, D=10, warmup=1, eps=0.0, daily=4096, ds=10, obs=4096, os_=10, drop=None, weight=None,
         count=0.0, count_dev=None, loss=4096, grad=None, terms=None, work=4096, desc=True):
    d = _lib.ObjectiveDesc(kind, 0, G, D, warmup, eps)
    return lib.ddr_daily_objective_f32(C.byref(d) if desc else None, daily, ds, obs, os_, drop, weight, count,
                                       count_dev, loss, grad, terms, work, None)


def test_c_abi_refuses_bad_arguments():
    """ddr_daily_objective_f32 checks its arguments before any launch: no device needed.  (The pointers are never
    dereferenced: every call below is refused, or a no-op.)"""
    lib = _lib.load()
    assert call(lib, G=0) == _lib.DDR_OK
    assert call(lib, G=0, D=100000, daily=None, obs=None, loss=None, work=None) == _lib.DDR_OK
    assert call(lib, desc=False) == _lib.DDR_ERR_ARG and b"descriptor" in lib.ddr_last_error()
    for kw in (dict(G=-1), dict(D=-1), dict(warmup=-1), dict(ds=-1), dict(os_=-1)):
        assert call(lib, **kw) == _lib.DDR_ERR_ARG, kw
        assert b"negative" in lib.ddr_last_error()
    for D in (0, 8193, 1 << 40):
        assert call(lib, D=D, warmup=0) == _lib.DDR_ERR_ARG
        assert b"8192" in lib.ddr_last_error()
    for warmup in (10, 11, 1 << 40):
        assert call(lib, warmup=warmup) == _lib.DDR_ERR_ARG
        assert b"warmup" in lib.ddr_last_error()
    for kind in (-1, 4, 1 << 20):
        assert call(lib, kind=kind) == _lib.DDR_ERR_ARG
        assert b"kind" in lib.ddr_last_error()
    for eps in (-1e-12, float("nan")):
        assert call(lib, eps=eps) == _lib.DDR_ERR_ARG
        assert b"eps" in lib.ddr_last_error()
    for count in (-1.0, float("nan")):
        assert call(lib, count=count) == _lib.DDR_ERR_ARG
        assert b"count" in lib.ddr_last_error()
    for name in ("daily", "obs", "loss", "work"):
        assert call(lib, **{name: None}) == _lib.DDR_ERR_ARG
        assert b"null " + name.encode() in lib.ddr_last_error()
    assert call(lib, G=(1 << 24) + 1) == _lib.DDR_ERR_ARG and b"gauges" in lib.ddr_last_error()


def test_work_bytes():
    lib = _lib.load()
    assert lib.ddr_daily_objective_work_bytes(-1) == -1
    assert lib.ddr_daily_objective_work_bytes((1 << 24) + 1) == -1
    sizes = [lib.ddr_daily_objective_work_bytes(G) for G in (0, 1, 2, 256, 1025)]
    assert sizes[0] >= 8 and all(b > a for a, b in zip(sizes, sizes[1:])) and all(s % 8 == 0 for s in sizes)
    assert (sizes[2] - sizes[1]) * 1023 == sizes[4] - sizes[2]  # linear in G


def test_header_binding_and_library_agree():
    text = header_code()
    lib = _lib.load()
    for name in FUNCTIONS:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.EXPORTED and hasattr(lib, name)
    # the argument list of the call, type by type
    params = re.search(r"ddr_status\s+ddr_daily_objective_f32\s*\(([^)]*)\)", text).group(1)
    want = []
    for prm in (s.strip() for s in params.split(",")):
        if "*" in prm:
            want.append(C.POINTER(_lib.ObjectiveDesc) if "ddr_objective_desc" in prm else C.c_void_p)
        else:
            want.append(CTYPES[prm.split()[0]])
    res, args = _lib._SIGS["ddr_daily_objective_f32"]
    assert res is C.c_int and args == want
    assert _lib._SIGS["ddr_daily_objective_work_bytes"] == (C.c_int64, [C.c_int64])
    # the descriptor, field by field
    body = re.search(r"typedef\s+struct\s+ddr_objective_desc\s*\{([^}]*)\}", text).group(1)
    fields = []
    for decl in (s.strip() for s in body.split(";") if s.strip()):
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), CTYPES[ctype]) for n in names.split(",")]
    assert fields == list(_lib.ObjectiveDesc._fields_)
    # the kinds, in the enum's order
    enum = re.search(r"enum\s*\{([^}]*DDR_OBJECTIVE_[^}]*)\}", text).group(1)
    names = [m.lower() for m in re.findall(r"DDR_OBJECTIVE_([A-Z0-9]+)", enum)]
    assert tuple(names) == tuple(OBJECTIVE_KINDS) == _lib.OBJECTIVE_KINDS
    assert re.search(r"DDR_OBJECTIVE_L1\s*=\s*0\b", enum) and "DDR_N_OBJECTIVES" in enum
