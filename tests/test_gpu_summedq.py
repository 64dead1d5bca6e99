"""The summed-Q' baseline on the device (csrc/summedq.hip) against tests/golden/summedq.npz: the reference's
arithmetic restated in NumPy (fp32 mean of 24, fp32 nansum) and an fp64 model of the definition.

Two derived bounds, on every element, with u = 2^-24, M the list length and S the fp64 sum of |daily| over the
list's non-NaN members (an element that equals its counterpart exactly, +inf included, passes as it is):

    |pred - model| <= u |model| + M 2^-53 S + 2^-149      one fp32 rounding, the fp64 reorderings, the denormal floor
    |pred - ref|   <= (M + 25) u S                        the reference's fp32 mean (24 u) and nansum ((M - 1) u), + u
"""

import numpy as np
import pytest
import torch

from conftest import load_golden
from ddr_amd.capture import CapturedStep
from ddr_amd.validation import METRIC_NAMES, Metrics, SummedQPrime, metrics_device, summed_q_prime_metrics

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
HOURLY_T = (24, 25, 47, 24 * 63, 24 * 64 + 5, 24 * 65)
DAILY_D = (1, 3, 63, 64, 65, 255, 256, 257, 1031)


@pytest.fixture(scope="module")
def golden():
    return load_golden("summedq")


def daily_fp64(qr: np.ndarray, rho: int) -> np.ndarray:
    n, T = qr.shape
    D = T // rho
    x = qr[:, : D * rho].astype(np.float64).reshape(n, D, rho)
    s = x[:, :, 0].copy()
    for h in range(1, rho):
        s += x[:, :, h]
    return s / rho if rho > 1 else s


def model_fp64(qr, rho, off, idx):
    """The definition in fp64, members in list order, and S = the sum of |daily| over the non-NaN members."""
    with np.errstate(all="ignore"):
        daily = daily_fp64(qr, rho)
        clean = np.where(np.isnan(daily), 0.0, daily)
        pred = np.zeros((len(off) - 1, daily.shape[1]))
        S = np.zeros_like(pred)
        for g in range(len(off) - 1):
            for i in idx[off[g]:off[g + 1]]:
                pred[g] += clean[i]
                S[g] += np.abs(clean[i])
    return pred, S


def reference_arithmetic(qr, rho, off, idx):
    """Lines 230, 232 and 259 of the reference script in its dtypes (as tests/golden/make_summedq_golden.py)."""
    n, T = qr.shape
    with np.errstate(all="ignore"):
        if rho == 24:
            daily = qr[:, : T // 24 * 24].reshape(n, T // 24, 24).mean(axis=2).astype(np.float32)
        else:
            daily = qr.astype(np.float32)
        return np.stack([np.nansum(daily[idx[off[g]:off[g + 1]]], axis=0) for g in range(len(off) - 1)])


def assert_bounds(pred: np.ndarray, model: np.ndarray, ref: np.ndarray, S: np.ndarray, off: np.ndarray, what: str):
    assert pred.dtype == np.float32 and pred.shape == model.shape == ref.shape == S.shape
    assert not np.isnan(model).any() and not np.isnan(ref).any()
    M = np.diff(off)[:, None].astype(np.float64)
    p = pred.astype(np.float64)
    with np.errstate(all="ignore"):
        err_m, err_r = np.abs(p - model), np.abs(p - ref.astype(np.float64))
        bound_m = U * np.abs(model) + M * 2.0 ** -53 * S + 2.0 ** -149
        bound_r = (M + 25.0) * U * S
        ok_m = (p == model) | (err_m <= bound_m)
        ok_r = (p == ref) | (err_r <= bound_r)
        finite = np.isfinite(model) & (model != 0)
        worst_m = float(np.max(np.where(finite, err_m / np.where(finite, np.abs(model), 1.0), 0.0))) / U
        worst_r = float(np.max(np.where(finite, err_r / np.where(finite, S, 1.0), 0.0))) / U
    print(f"{what}: worst |pred - model| = {worst_m:.3f} u |model|, worst |pred - ref| = {worst_r:.3f} u S")
    assert ok_m.all(), (what, "model", np.argwhere(~ok_m)[:8].tolist(), p[~ok_m][:8], model[~ok_m][:8])
    assert ok_r.all(), (what, "reference", np.argwhere(~ok_r)[:8].tolist(), p[~ok_r][:8], ref[~ok_r][:8])


def run_case(golden, tag, cuda, chunk=4096):
    qr = golden[str(golden[f"store_{tag}"])][:, : int(golden[f"T_{tag}"])]
    rho = int(golden[f"rho_{tag}"])
    off, idx = golden[f"off_{tag}"], golden[f"idx_{tag}"]
    summed = SummedQPrime(off, idx, device=cuda, chunk=chunk)
    pred = summed(torch.from_numpy(np.ascontiguousarray(qr)).to(cuda), rho)
    assert pred.dtype == torch.float32 and pred.device == cuda and pred.shape == golden[f"model_{tag}"].shape
    _, S = model_fp64(qr, rho, off, idx)
    assert_bounds(pred.cpu().numpy(), golden[f"model_{tag}"], golden[f"ref_{tag}"], S, off, f"{tag} chunk {chunk}")
    return pred


@pytest.mark.parametrize("tag", [f"h{T}" for T in HOURLY_T] + [f"d{D}" for D in DAILY_D])
def test_fixture_cases(cuda, golden, tag):
    run_case(golden, tag, cuda)


@pytest.mark.parametrize("tag", ["lists_d", "lists_h"])
def test_list_lengths_around_the_chunk(cuda, golden, tag):
    """Lists of 0, 1, 7, 8, 9, 16, 17 and 27 members with chunk = 8: one, two, three and four pieces; different
    chunks may differ in the last fp64 bits and both meet the bounds."""
    assert np.diff(golden[f"off_{tag}"]).tolist() == [0, 1, 7, 8, 9, 16, 17, 27]
    small = run_case(golden, tag, cuda, chunk=8)
    whole = run_case(golden, tag, cuda)
    assert (small[0] == 0).all() and (whole[0] == 0).all()  # the empty list
    assert torch.equal(small[:4], whole[:4])  # up to 8 members nothing is split


def test_list_of_two_chunks_and_one_member(cuda, golden):
    """2 * 4096 + 1 members at D = 70 with the default chunk: three pieces.  From the fixture (members repeat), and
    on 8193 distinct rows of a 9000-row store."""
    run_case(golden, "big", cuda)
    rng = np.random.default_rng(11)
    qr = (rng.lognormal(np.log(0.5), 1.0, (9000, 1)) * rng.lognormal(0.0, 0.5, (9000, 70))).astype(np.float32)
    qr[rng.integers(0, 9000, 40), rng.integers(0, 70, 40)] = np.nan
    off = np.array([0, 8193, 8193 + 4096], np.int64)
    idx = np.concatenate([rng.permutation(9000)[:8193], rng.permutation(9000)[:4096]]).astype(np.int32)
    summed = SummedQPrime(off, idx, device=cuda)
    assert summed.scratch_bytes(70) == 3 * 70 * 8  # the second list is exactly one chunk: not split
    pred = summed(torch.from_numpy(qr).to(cuda), 1).cpu().numpy()
    model, S = model_fp64(qr, 1, off, idx)
    assert_bounds(pred, model, reference_arithmetic(qr, 1, off, idx), S, off, "8193 of 9000 rows")


def test_special_rows(cuda, golden):
    qr = golden["qr_long"][:, : 24 * 65]
    rows = dict(zip(golden["special_names"].tolist(), golden["special_rows"].tolist()))
    r_nan, r_all, r_inf = rows["nan_hours"], rows["all_nan"], rows["plus_inf"]
    lists = [[r_nan], [r_all], [r_nan, r_all], [0], [0, r_all], [r_inf, 2], [2, r_nan, 0]]
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(m) for m in lists], out=off[1:])
    idx = np.array([i for m in lists for i in m], np.int32)
    dev = torch.from_numpy(np.ascontiguousarray(qr)).to(cuda)
    summed = SummedQPrime(off, idx, device=cuda)
    for rho in (24, 1):
        pred = summed(dev, rho).cpu().numpy()
        with np.errstate(all="ignore"):
            daily = daily_fp64(qr, rho)
        nan_days = np.isnan(daily[r_nan])
        assert nan_days.any() and not nan_days.all()
        # a NaN hour makes that member's day count as 0; the rest of its days count
        assert (pred[0][nan_days] == 0.0).all()
        assert np.array_equal(pred[0][~nan_days], daily[r_nan][~nan_days].astype(np.float32))
        assert np.array_equal(pred[6][nan_days], (daily[2] + daily[0]).astype(np.float32)[nan_days])
        assert np.array_equal(pred[6][~nan_days], (daily[2] + daily[r_nan] + daily[0]).astype(np.float32)[~nan_days])
        # a member that is NaN throughout adds nothing; a gauge that is all NaN on a day gives exactly 0.0
        assert (pred[1] == 0.0).all() and not np.signbit(pred[1]).any()
        assert np.array_equal(pred[2], pred[0])
        assert np.array_equal(pred[4], pred[3]) and (pred[3] > 0).all()
        # +inf follows IEEE
        inf_days = np.isposinf(daily[r_inf])
        assert inf_days.any() and np.isposinf(pred[5][inf_days]).all() and np.isfinite(pred[5][~inf_days]).all()


def test_trailing_hours_are_ignored(cuda, golden):
    T = 24 * 64 + 5
    qr = np.ascontiguousarray(golden["qr_long"][:, :T])
    off, idx = golden[f"off_h{T}"], golden[f"idx_h{T}"]
    summed = SummedQPrime(off, idx, device=cuda)
    dev = torch.from_numpy(qr).to(cuda)
    pred = summed(dev, 24)
    assert pred.shape == (len(off) - 1, 64)
    filled = dev.clone()
    filled[:, 24 * 64:] = float("nan")
    assert torch.equal(summed(filled, 24), pred)
    assert torch.equal(summed(dev[:, : 24 * 64], 24), pred)  # (a view with the same row stride)


@pytest.mark.parametrize("rho", [24, 1])
def test_strides_equal_the_contiguous_call(cuda, golden, rho):
    """Views go through the 16-byte path when base and row stride allow it and the 4-byte path otherwise; the
    values are the same bit for bit."""
    T = 24 * 65
    qr = torch.from_numpy(np.ascontiguousarray(golden["qr_long"][:, :T])).to(cuda)
    n = qr.shape[0]
    off, idx = golden[f"off_h{T}"], golden[f"idx_h{T}"]
    summed = SummedQPrime(off, idx, device=cuda)
    want = summed(qr, rho)
    assert qr.data_ptr() % 16 == 0 and qr.stride(0) % 4 == 0  # the contiguous call takes 16-byte loads

    def padded(front, back=0):
        wide = torch.full((n, front + T + back), float("nan"), device=cuda)
        wide[:, front:front + T] = qr
        return wide[:, front:front + T]

    aligned = padded(24)  # a time slice of a wider store: keeps 16-byte alignment
    assert aligned.data_ptr() % 16 == 0 and aligned.stride(0) % 4 == 0 and not aligned.is_contiguous()
    shifted = padded(1)  # breaks it
    assert shifted.data_ptr() % 16 == 4
    odd = padded(0, 3)  # an odd row stride
    assert odd.data_ptr() % 16 == 0 and odd.stride(0) % 2 == 1
    transposed = qr.t().contiguous().t()  # innermost stride != 1: made contiguous
    assert transposed.stride(1) != 1
    for name, view in (("aligned", aligned), ("shifted", shifted), ("odd", odd), ("transposed", transposed)):
        assert torch.equal(view.contiguous().view(torch.int32), qr.view(torch.int32)), name  # (bits: NaN rows)
        assert torch.equal(summed(view, rho), want), name


@pytest.mark.parametrize("tag", ["lists_d", "lists_h"])
def test_a_gauge_row_does_not_depend_on_its_batch(cuda, golden, tag):
    qr = torch.from_numpy(np.ascontiguousarray(golden["qr_lists"])).to(cuda)
    rho = int(golden[f"rho_{tag}"])
    off, idx = golden[f"off_{tag}"], golden[f"idx_{tag}"]
    G = len(off) - 1
    lists = [idx[off[g]:off[g + 1]] for g in range(G)]

    def plan(gauges, chunk):
        o = np.zeros(len(gauges) + 1, np.int64)
        np.cumsum([len(lists[g]) for g in gauges], out=o[1:])
        return SummedQPrime(o, np.concatenate([lists[g] for g in gauges]).astype(np.int32), device=cuda, chunk=chunk)

    for chunk in (4096, 8):
        full = plan(range(G), chunk)(qr, rho)
        assert torch.equal(plan(range(G), chunk)(qr, rho), full)  # a second plan, a second call
        assert torch.equal(full, plan(range(G), chunk)(qr, rho))
        for g in range(G):  # alone (chunk = 8 against chunk = 8 with the other gauges removed)
            assert torch.equal(plan([g], chunk)(qr, rho)[0], full[g]), (chunk, g)
        perm = [5, 0, 7, 2, 6, 1, 4, 3]
        assert torch.equal(plan(perm, chunk)(qr, rho), full[perm]), chunk
        assert torch.equal(plan([7, 6], chunk)(qr, rho), full[[7, 6]]), chunk


def test_hand_off_to_the_metrics(cuda, golden):
    tag = "lists_d"
    qr = torch.from_numpy(np.ascontiguousarray(golden["qr_lists"])).to(cuda)
    off, idx = golden[f"off_{tag}"][1:], golden[f"idx_{tag}"]  # (without the empty gauge: its NSE is degenerate)
    summed = SummedQPrime(off, idx, device=cuda, chunk=8)
    model = golden[f"model_{tag}"][1:]
    rng = np.random.default_rng(3)
    target_np = (model * np.exp(rng.normal(0.0, 0.2, model.shape))).astype(np.float32)
    target_np[rng.uniform(size=model.shape) < 0.05] = np.nan
    target = torch.from_numpy(target_np).to(cuda)
    pred, values, count = summed_q_prime_metrics(summed, qr, target, hours_per_step=1, warmup=2)
    assert torch.equal(pred, summed(qr, 1)) and int(count.item()) == 0
    separate, _ = metrics_device(pred, target, warmup=2)
    assert torch.equal(values, separate)
    m = Metrics(pred.cpu().numpy()[:, 2:], target_np[:, 2:])
    nse = values[METRIC_NAMES.index("nse")].cpu().numpy()
    assert np.isfinite(nse).all()
    assert np.array_equal(m.nse, nse)


@pytest.mark.parametrize("rho,chunk", [(24, 4096), (1, 8)])
def test_captured_call_replays_on_changed_contents(cuda, golden, rho, chunk):
    """One call captured by torch.cuda.graph (one launch, two with split lists) and replayed on new qr contents."""
    host = np.ascontiguousarray(golden["qr_lists"])
    off, idx = golden["off_lists_d"], golden["idx_lists_d"]
    summed = SummedQPrime(off, idx, device=cuda, chunk=chunk)
    qr = torch.from_numpy(host).to(cuda)
    box = {}

    def step():
        box["pred"] = summed(qr, rho)

    captured = CapturedStep(step, warmup=1, device=cuda)
    rng = np.random.default_rng(8)
    for _ in range(2):
        fresh = torch.from_numpy((host * rng.lognormal(0.0, 0.3, host.shape)).astype(np.float32)).to(cuda)
        qr.copy_(fresh)
        captured()
        assert torch.equal(box["pred"], summed(fresh, rho))
