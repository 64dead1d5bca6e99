"""Generate ``summedq.npz``: inputs, the reference's arithmetic and an fp64 model of the summed-Q' baseline.

The reference's ``scripts/summed_q_prime.py`` imports CuPy, hydra and xarray at module level and cannot be imported
without them, so its three arithmetic lines (230, 232 and 259) are restated here in NumPy:

    qr_daily = qr[:, :days * 24].reshape(n, days, 24).mean(axis=2)        float32 in, float32 mean
    qr_daily = qr_daily.astype(np.float32)
    pred[g]  = np.nansum(qr_daily[idx_g], axis=0)                         float32 (cp.nansum on the device)

Parity is therefore pinned to this NumPy restatement, not to a CuPy run.  Next to it the file stores an fp64 model
of the definition: the hours of a day added in hour order and divided by 24, the members added in list order, NaN
days skipped, nothing rounded to fp32.

Inputs are positive and log-normal, a scale per divide times hourly noise (the law of
``ddr_amd.synthetic.lateral_inflow`` without its smooth shape, so that the mantissas are random).  Two stores:

* ``qr_long`` (10, 1565): rows 6, 7 and 8 are special -- NaN at single hours, NaN throughout, +inf at single hours.
  Cases ``h<T>`` read its first T hours as an hourly store, cases ``d<D>`` its first D columns as a daily store.
  Gauges: 0 = ten rows with both NaN rows among them, 1 = the two NaN rows alone (days on which both are NaN must
  give exactly 0), 2 = three rows with the +inf row, 3 = a single row.
* ``qr_lists`` (40, 72): row 5 has NaN hours, row 11 is NaN throughout.  Cases ``lists_d`` (daily) and ``lists_h``
  (hourly) hold lists of 0, 1, 7, 8, 9, 16, 17 and 27 distinct members in shuffled order: with chunk = 8 these sit
  on and around one, two and three pieces.
* Case ``big``: 2 * 4096 + 1 members drawn with repetition from the rows of ``qr_long[:, :70]`` as a daily store:
  three pieces at the default chunk.

Keys: ``cases`` the tags; per tag ``store_<tag>`` (name of the store), ``rho_<tag>``, ``T_<tag>``, ``off_<tag>``
int64, ``idx_<tag>`` int32, ``ref_<tag>`` (G, D) float32 the reference's arithmetic, ``model_<tag>`` (G, D) float64;
``special_names`` with ``special_rows`` (row of ``qr_long``) for the three special rows.

The maker asserts that the reference's arithmetic is within (M + 24) u S of the model on every element (u = 2^-24,
M the list length, S the sum of |daily| over the non-NaN members).

Run:  python tests/golden/make_summedq_golden.py
"""

from __future__ import annotations

from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
U = 2.0 ** -24

HOURLY_T = (24, 25, 47, 24 * 63, 24 * 64 + 5, 24 * 65)
DAILY_D = (1, 3, 63, 64, 65, 255, 256, 257, 1031)
LIST_LENGTHS = (0, 1, 7, 8, 9, 16, 17, 27)
BIG_MEMBERS = 2 * 4096 + 1
SPECIAL = ("nan_hours", "all_nan", "plus_inf")
SPECIAL_ROWS = (6, 7, 8)
NAN_HOURS = (0, 2, 30, 47, 70, 254, 255, 256, 1030, 24 * 62 + 3, 24 * 63 + 23, 24 * 64 + 7)
INF_HOURS = (1, 50, 64, 300, 24 * 63 + 1)
LONG_LISTS = ([0, 1, 2, 3, 4, 5, 6, 7, 9, 3], [6, 7], [9, 8, 2], [5])


def lognormal_store(rng: np.random.Generator, n: int, T: int) -> np.ndarray:
    scale = rng.lognormal(np.log(0.5), 1.0, (n, 1))
    return (scale * rng.lognormal(0.0, 0.5, (n, T))).astype(np.float32)


def csr(lists) -> tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(m) for m in lists], out=off[1:])
    idx = np.concatenate([np.asarray(m, np.int32) for m in lists]) if off[-1] else np.zeros(0, np.int32)
    return off, idx.astype(np.int32)


def reference_arithmetic(qr: np.ndarray, rho: int, off: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """Lines 230, 232 and 259 of the reference script, in its dtypes."""
    n, T = qr.shape
    if rho == 24:
        days = T // 24
        daily = qr[:, : days * 24].reshape(n, days, 24).mean(axis=2)
        daily = daily.astype(np.float32)
    else:
        daily = qr.astype(np.float32)
    pred = np.zeros((len(off) - 1, daily.shape[1]), np.float32)
    for g in range(len(off) - 1):
        pred[g] = np.nansum(daily[idx[off[g]:off[g + 1]]], axis=0)
    return pred


def daily_fp64(qr: np.ndarray, rho: int) -> np.ndarray:
    n, T = qr.shape
    D = T // rho
    x = qr[:, : D * rho].astype(np.float64).reshape(n, D, rho)
    s = x[:, :, 0].copy()
    for h in range(1, rho):
        s += x[:, :, h]
    return s / rho if rho > 1 else s


def model_fp64(qr: np.ndarray, rho: int, off: np.ndarray, idx: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The definition in fp64, members in list order; and S, the sum of |daily| over the non-NaN members."""
    daily = daily_fp64(qr, rho)
    clean = np.where(np.isnan(daily), 0.0, daily)
    G = len(off) - 1
    pred = np.zeros((G, daily.shape[1]))
    S = np.zeros_like(pred)
    for g in range(G):
        for i in idx[off[g]:off[g + 1]]:
            pred[g] += clean[i]
            S[g] += np.abs(clean[i])
    return pred, S


def main() -> None:
    rng = np.random.default_rng(20259)
    qr_long = lognormal_store(rng, 10, 24 * 65 + 5)
    qr_long[6, list(NAN_HOURS)] = np.nan
    qr_long[7] = np.nan
    qr_long[8, list(INF_HOURS)] = np.inf
    qr_lists = lognormal_store(rng, 40, 72)
    qr_lists[5, [0, 3, 30, 71]] = np.nan
    qr_lists[11] = np.nan
    stores = {"qr_long": qr_long, "qr_lists": qr_lists}

    cases = []  # (tag, store, rho, T, lists)
    for T in HOURLY_T:
        cases.append((f"h{T}", "qr_long", 24, T, LONG_LISTS))
    for D in DAILY_D:
        cases.append((f"d{D}", "qr_long", 1, D, LONG_LISTS[:3] if D > 1000 else LONG_LISTS))
    member_lists = [rng.permutation(40)[:m].tolist() for m in LIST_LENGTHS]
    member_lists[5] = [5, 11] + [i for i in member_lists[5] if i not in (5, 11)][:14]  # both NaN rows in one list
    cases.append(("lists_d", "qr_lists", 1, 72, member_lists))
    cases.append(("lists_h", "qr_lists", 24, 72, member_lists))
    cases.append(("big", "qr_long", 1, 70, [rng.integers(0, 10, BIG_MEMBERS).tolist()]))

    out = {"cases": np.array([c[0] for c in cases]), "special_names": np.array(SPECIAL),
           "special_rows": np.array(SPECIAL_ROWS, np.int32), **stores}
    for tag, store, rho, T, lists in cases:
        qr = stores[store][:, :T]
        off, idx = csr(lists)
        with np.errstate(all="ignore"):
            ref = reference_arithmetic(qr, rho, off, idx)
            model, S = model_fp64(qr, rho, off, idx)
            M = np.diff(off)[:, None].astype(np.float64)
            err = np.abs(ref.astype(np.float64) - model)
            ok = (ref.astype(np.float64) == model) | (err <= (M + 24.0) * U * S)
        assert ok.all(), (tag, float(np.nanmax(np.where(ok, 0.0, err))))
        assert ref.shape == model.shape == (len(lists), T // rho)
        worst = float(np.nanmax(np.where(np.isfinite(S) & (S > 0), err / (U * np.where(S > 0, S, 1.0)), 0.0)))
        print(f"{tag}: G={len(lists)} D={T // rho} reference within {worst:.2f} u S of the model "
              f"(allowed M + 24), zeros {int((model == 0).sum())}, inf {int(np.isinf(model).sum())}")
        out[f"store_{tag}"], out[f"rho_{tag}"], out[f"T_{tag}"] = np.array(store), np.int64(rho), np.int64(T)
        out[f"off_{tag}"], out[f"idx_{tag}"], out[f"ref_{tag}"], out[f"model_{tag}"] = off, idx, ref, model
    path = HERE / "summedq.npz"
    np.savez_compressed(path, **out)
    size, limit = path.stat().st_size, (HERE / "metrics.npz").stat().st_size
    print("wrote", path, size, "bytes (metrics.npz:", limit, ")")
    assert size <= limit


if __name__ == "__main__":
    main()
