"""Drop-in for ``ddr.geometry.adapters`` (reference ``src/ddr/geometry/adapters.py:22-168``) without xarray.

The KAN is trained on MERIT-Hydro catchment attributes; another source (HydroATLAS) has the same ten quantities
under other names and, for the upstream area, in other units.  The reference converts them on the host in fp64;
here :func:`adapt_attributes` only *selects and orders* the columns and hands back the per-feature
``(scale, offset, log10)`` that ``attr_prepare_kernel`` (``csrc/geopredict.hip``) applies on the device, in
fp64 like the reference, on its way to the KAN's input.
"""

from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

log = logging.getLogger(__name__)

# the KAN's native inputs, in its order
MERIT_ATTRIBUTE_NAMES = ("SoilGrids1km_clay", "aridity", "meanelevation", "meanP", "NDVI", "meanslope", "log10_uparea",
                         "SoilGrids1km_sand", "ETPOT_Hargr", "Porosity")


@dataclass(frozen=True)
class AttributeMapping:
    """One external attribute -> its MERIT equivalent: ``value * scale + offset``, then ``log10`` (of the value
    clipped to >= 1e-6) when ``log_transform``."""

    merit_name: str
    scale: float = 1.0
    offset: float = 0.0
    log_transform: bool = False


def _m(name: str, **kw) -> AttributeMapping:
    return AttributeMapping(merit_name=name, **kw)


HYDROATLAS_TO_MERIT: dict[str, AttributeMapping] = {
    "cly_pc_sav": _m("SoilGrids1km_clay"), "ari_ix_sav": _m("aridity"), "ele_mt_sav": _m("meanelevation"),
    "pre_mm_syr": _m("meanP"), "ndv_ix_sav": _m("NDVI"), "slp_dg_sav": _m("meanslope"),
    "upa_sk_smx": _m("log10_uparea", log_transform=True), "snd_pc_sav": _m("SoilGrids1km_sand"),
    "pet_mm_syr": _m("ETPOT_Hargr"), "por_pc_sav": _m("Porosity"),
}

_KNOWN_SOURCES: dict[str, dict[str, AttributeMapping]] = {"hydroatlas": HYDROATLAS_TO_MERIT}


class AdaptedAttributes(NamedTuple):
    """What :func:`adapt_attributes` returns: ``columns[name]`` is the source's (N,) array for the MERIT attribute
    ``name`` (untransformed), in ``MERIT_ATTRIBUTE_NAMES`` order; ``scale`` / ``offset`` (fp64) and ``log10``
    (int32) are the per-feature transform the prepare kernel applies, in the same order."""

    columns: dict
    scale: np.ndarray
    offset: np.ndarray
    log10: np.ndarray
    source: str


def _names(attrs) -> set:
    """The variable names of a mapping (or of an ``xarray.Dataset``: its ``data_vars``)."""
    return set(getattr(attrs, "data_vars", attrs))


def detect_source(attrs) -> str | None:
    """``"merit"``, a registered external source (``"hydroatlas"``), or None, from the variable names of a
    mapping, a Dataset or any iterable of names."""
    names = _names(attrs)
    if names >= set(MERIT_ATTRIBUTE_NAMES):
        return "merit"
    for source, mapping in _KNOWN_SOURCES.items():
        if names >= set(mapping):
            return source
    return None


def adapt_attributes(attrs, source: str = "auto") -> AdaptedAttributes:
    """Select the ten attributes of ``attrs`` (a mapping name -> (N,) array-like; an ``xarray.Dataset`` works
    through the same ``attrs[name]`` access) under their MERIT names and order, with the transform that turns
    each into MERIT units.  Nothing is computed here.

    Raises ``ValueError`` for an undetectable source, an unknown source, or missing variables (named in the
    message), as the reference does."""
    names = _names(attrs)
    if source == "auto":
        source = detect_source(names)
        if source is None:
            raise ValueError(f"Cannot auto-detect attribute source from variables: {sorted(names)}. Expected MERIT "
                             f"names {MERIT_ATTRIBUTE_NAMES} or HydroATLAS names {sorted(HYDROATLAS_TO_MERIT)}. "
                             "Specify source='merit' or source='hydroatlas'.")
    if source == "merit":
        mapping = {name: AttributeMapping(merit_name=name) for name in MERIT_ATTRIBUTE_NAMES}
        label = "MERIT"
    else:
        mapping = _KNOWN_SOURCES.get(source)
        label = source
        if mapping is None:
            raise ValueError(f"Unknown attribute source: {source!r}. Known sources: {sorted(_KNOWN_SOURCES)}")
    missing = set(mapping) - names
    if missing:
        raise ValueError(f"Missing {label} attributes: {sorted(missing)}")
    by_merit = {m.merit_name: (src, m) for src, m in mapping.items()}
    ordered = [by_merit[name] for name in MERIT_ATTRIBUTE_NAMES]
    if source != "merit":
        log.info("Converted %d attributes from %s to MERIT format", len(ordered), source)
    return AdaptedAttributes(
        columns={m.merit_name: attrs[src] for src, m in ordered},
        scale=np.array([m.scale for _, m in ordered], dtype=np.float64),
        offset=np.array([m.offset for _, m in ordered], dtype=np.float64),
        log10=np.array([int(m.log_transform) for _, m in ordered], dtype=np.int32),
        source=source)
