"""The host half of whole-period inference (ddr_amd/inference.py): the chunk plan of the reference's ``ddr route`` /
``ddr test`` loop, its argument errors, and the fixture tests/golden/period.npz (the reference's own loop,
make_period_golden.py) against the same loop composed from the CPU oracle.

Bars: routed discharge against a reference golden 1e-4 max-rel (tests/test_gpu_state.py); the reference and the
oracle agree to ~5e-7 (daily) and ~7e-7 (hourly) on this case, while two chunkings of the same period differ by
2.4e-3 -- the plan is part of the result.
"""

import numpy as np
import pytest

from conftest import maxrel
from ddr_amd.inference import PeriodRouter, period_chunks
from period_helpers import CHUNK_DAYS, MODES, TAUS, oracle_period, period_case, reference_chunks

N_DAYS = (3, 8, 9, 366)
BATCHES = (2, 3, 7, 8, 400)


@pytest.mark.parametrize("n_days", N_DAYS)
@pytest.mark.parametrize("B", BATCHES)
def test_chunks_tile_the_period(n_days, B):
    chunks = period_chunks(n_days, B)
    assert chunks == reference_chunks(n_days, B)
    hour = 0
    for k, (first, last) in enumerate(chunks):
        assert first * 24 == hour, "chunks must be contiguous and must not overlap"
        assert last > first
        hour = last * 24
        hours = (last - first) * 24
        new_days = min((k + 1) * B, n_days) - k * B  # the sampler's batch, before the previous day is prepended
        assert hours == (new_days - 1) * 24 if k == 0 else hours == new_days * 24
    assert hour == (n_days - 1) * 24
    first_full = min(B, n_days)
    assert (chunks[0][1] - chunks[0][0]) * 24 == (first_full - 1) * 24
    for first, last in chunks[1:-1]:
        assert (last - first) * 24 == B * 24
    if n_days > B and n_days % B == 1:  # a trailing chunk of one new day
        assert chunks[-1] == (n_days - 2, n_days - 1)


@pytest.mark.parametrize("B", CHUNK_DAYS)
def test_chunks_match_the_reference_run(B):
    _, store, _, d = period_case()
    assert period_chunks(store.shape[0], B) == [tuple(int(v) for v in row) for row in d[f"chunks_B{B}"]]


def test_argument_errors():
    for B in (1, 0, -3):
        with pytest.raises(ValueError):
            period_chunks(8, B)
    for n_days in (2, 1, 0):
        with pytest.raises(ValueError):
            period_chunks(n_days, 3)
    for tau in (-1, 11):
        with pytest.raises(ValueError):
            PeriodRouter(None, None, None, None, chunk_days=3, tau=tau)
    with pytest.raises(ValueError):
        PeriodRouter(None, None, None, None, chunk_days=1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("B", CHUNK_DAYS)
def test_fixture_agrees_with_the_oracle_composition(B, tau, mode):
    _, _, _, d = period_case()
    daily, hourly = oracle_period(B, tau, mode)
    ref = d[f"daily_B{B}_tau{tau}_{mode}"]
    assert daily.shape == ref.shape
    err = maxrel(daily, ref)
    print(f"B={B} tau={tau} {mode}: daily max-rel {err:.3e}")
    assert err <= 1e-4
    if B == 3:
        err = maxrel(hourly, d[f"hourly_B3_{mode}"])
        print(f"B={B} {mode}: hourly max-rel {err:.3e}")
        assert err <= 1e-4


def test_the_chunking_is_part_of_the_result():
    """Two plans over the same period differ by far more than the parity bar, so a port that routed the period in one
    piece (or with another plan) would fail the parity tests."""
    _, _, _, d = period_case()
    assert maxrel(d["daily_B3_tau3_all"], d["daily_B8_tau3_all"]) > 1e-3
    assert maxrel(oracle_period(3, 3, "all")[0], oracle_period(8, 3, "all")[0]) > 1e-3
