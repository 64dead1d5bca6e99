"""Generate ``rapid_sandbox.npz`` from RAPID2's published Sandbox case (data only).

    python tests/golden/make_rapid_golden.py <reference checkout>

reads ``tests/input/Sandbox/{Qext,Qinit}_Sandbox_19700101_19700110.nc4`` and
``tests/output/Sandbox/{Qout,Qfinal}_Sandbox_19700101_19700110.nc4`` below the given directory: 5 reaches, 80
three-hourly forcings, 12 sub-steps of 900 s, k = 9000 s, x = 0.25.  The files are netCDF-4 (HDF5) with
contiguous, uncompressed datasets: a reader is used when one imports, the byte offsets below otherwise, and the
landmarks are asserted either way.

Arrays: ``ids`` (5,) int64, ``next_down`` (5,) int64 (0: the outlet), ``k``, ``x``, ``dt`` float64 scalars,
``substeps`` int64, ``qext`` (80, 5) float32, ``qinit`` (5,) float64, ``qout`` (80, 5) float32, ``qfinal`` (5,)
float64.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
STEM = "_Sandbox_19700101_19700110.nc4"
# variable: (directory, dtype, byte offset of the contiguous dataset, shape)
FILES = {
    "Qext": ("input", "<f4", 36491, (80, 5)),
    "Qout": ("output", "<f4", 27681, (80, 5)),
    "Qfinal": ("output", "<f8", 18330, (1, 5)),
    "Qinit": ("input", "<f8", 24522, (1, 5)),
}


def read(root: Path, var: str) -> np.ndarray:
    where, dtype, offset, shape = FILES[var]
    path = root / "tests" / where / "Sandbox" / (var + STEM)
    try:
        import netCDF4  # type: ignore

        with netCDF4.Dataset(path) as ds:
            a = np.asarray(ds.variables[var][:]).astype(dtype)
    except ImportError:
        try:
            import h5py  # type: ignore

            with h5py.File(path, "r") as f:
                a = np.asarray(f[var][...]).astype(dtype)
        except ImportError:
            a = np.fromfile(path, dtype=dtype, count=int(np.prod(shape)), offset=offset)
    return a.reshape(shape)


def main(root: Path) -> None:
    qext = read(root, "Qext").astype(np.float32)
    qout = read(root, "Qout").astype(np.float32)
    qinit = read(root, "Qinit").astype(np.float64).reshape(5)
    qfinal = read(root, "Qfinal").astype(np.float64).reshape(5)
    assert np.array_equal(qinit, [9, 9, 27, 18, 63]), qinit
    for r in (0, 39):
        assert np.array_equal(qext[r], [11, 11, 11, 22, 22]), (r, qext[r])
    for r in (40, 79):
        assert np.array_equal(qext[r], [9, 9, 9, 18, 18]), (r, qext[r])
    assert np.allclose(qout[0], [9.935223, 9.935223, 28.294682, 19.870445, 65.38851], rtol=2e-7, atol=0), qout[0]
    assert np.all(np.isfinite(qout)) and np.all(np.isfinite(qfinal))
    np.savez(HERE / "rapid_sandbox.npz", ids=np.array([10, 20, 30, 40, 50], np.int64),
             next_down=np.array([30, 30, 50, 50, 0], np.int64), k=np.float64(9000.0), x=np.float64(0.25),
             dt=np.float64(900.0), substeps=np.int64(12), qext=qext, qinit=qinit, qout=qout, qfinal=qfinal)
    print("wrote", HERE / "rapid_sandbox.npz")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(Path(sys.argv[1]))
