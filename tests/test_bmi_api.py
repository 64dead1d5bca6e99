"""The BMI coupling's host side (no GPU needed): the C ABI's new entry points and their argument checks, the
``BmiInitConfig`` schema, and everything of ``ddr_amd.bmi.DdrBmi`` that runs before a device is touched -- the
variable / time / grid tables of the reference (``src/ddr/bmi/ddr_bmi.py:47-78, 332-501``, restated from its
``tests/bmi/test_ddr_bmi.py:178-271``), the errors before ``initialize``, the nexus mapping read from a GeoPackage
and ``update_until``'s step-count and time bookkeeping."""

import ctypes as C
import re
import sqlite3
from pathlib import Path

import numpy as np
import pytest

from ddr_amd import _lib
from ddr_amd.bmi import BmiInitConfig, DdrBmi
from ddr_amd.bmi.ddr_bmi import plan_interval

HEADER = Path(__file__).resolve().parents[1] / "include" / "ddr_mc.h"
ENTRY_POINTS = ("ddr_bmi_nexus_table", "ddr_bmi_nexus_plan", "ddr_bmi_set_inflow_f64", "ddr_bmi_window_f32",
                "ddr_bmi_outputs_f32")
Q = "channel_exit_water_x-section__volume_flow_rate"


# ---- the C ABI --------------------------------------------------------------------------------------------------
def test_entry_points_in_header_binding_and_library():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.EXPORTED, name
        assert hasattr(lib, name), name


def _refused(code, fragment):
    assert code == _lib.DDR_ERR_ARG
    assert fragment in _lib.load().ddr_last_error().decode(), _lib.load().ddr_last_error()


def test_nexus_table_checks_its_host_arrays():
    lib = _lib.load()
    keys = np.array([3, 7, 7, 9], np.int64)
    segs = np.array([0, 1, 2, 3], np.int32)
    fake = 4096  # (never dereferenced: every call below is refused before anything is copied or launched)
    _refused(lib.ddr_bmi_nexus_table(4, keys.ctypes.data, segs.ctypes.data, 4, fake, fake, None), "strictly ascending")
    keys = np.array([3, 7, 8, 9], np.int64)
    _refused(lib.ddr_bmi_nexus_table(4, keys.ctypes.data, segs.ctypes.data, 3, fake, fake, None), "outside [0, 3)")
    segs[1] = -1
    _refused(lib.ddr_bmi_nexus_table(4, keys.ctypes.data, segs.ctypes.data, 4, fake, fake, None), "outside [0, 4)")
    _refused(lib.ddr_bmi_nexus_table(-1, None, None, 4, None, None, None), "negative size")
    _refused(lib.ddr_bmi_nexus_table(4, None, segs.ctypes.data, 4, fake, fake, None), "null argument")
    _refused(lib.ddr_bmi_nexus_table(1, keys.ctypes.data, segs.ctypes.data, 1 << 31, fake, fake, None), "int32")


def test_kernel_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    fake = 4096
    _refused(lib.ddr_bmi_nexus_plan(-1, None, 0, None, None, 4, fake, None), "negative size")
    _refused(lib.ddr_bmi_nexus_plan(2, None, 1, fake, fake, 4, fake, None), "null argument")
    _refused(lib.ddr_bmi_nexus_plan(2, fake, 1, fake, None, 4, fake, None), "null argument")
    _refused(lib.ddr_bmi_nexus_plan(2, fake, 1, fake, fake, 4, None, None), "null argument")
    _refused(lib.ddr_bmi_nexus_plan(1 << 31, fake, 1, fake, fake, 4, fake, None), "int32")
    _refused(lib.ddr_bmi_set_inflow_f64(4, fake, -1, fake, fake, None), "negative size")
    _refused(lib.ddr_bmi_set_inflow_f64(4, None, 2, fake, fake, None), "null argument")
    _refused(lib.ddr_bmi_set_inflow_f64(4, fake, 2, fake, None, None), "null argument")
    _refused(lib.ddr_bmi_window_f32(4, 0, 4, 0, fake, fake, fake, 4, None), "1 <= n_rows <= n_steps")
    _refused(lib.ddr_bmi_window_f32(4, 5, 4, 1, fake, fake, fake, 4, None), "1 <= n_rows <= n_steps")
    _refused(lib.ddr_bmi_window_f32(-4, 1, 1, 0, fake, fake, fake, 4, None), "negative size")
    _refused(lib.ddr_bmi_window_f32(4, 1, 1, 0, fake, fake, fake, 3, None), "row_stride")
    _refused(lib.ddr_bmi_window_f32(4, 1, 1, 0, fake, None, fake, 4, None), "null argument")
    args = [fake] * 4 + [1] + [fake] * 3 + [0.01, 0.01, fake, 4, None]
    _refused(lib.ddr_bmi_outputs_f32(-1, *args), "negative size")
    _refused(lib.ddr_bmi_outputs_f32(4, *args[:4], 2, *args[5:]), "p_stride")
    _refused(lib.ddr_bmi_outputs_f32(4, *args[:11], 3, None), "out_stride")
    _refused(lib.ddr_bmi_outputs_f32(4, None, *args[1:]), "null argument")
    _refused(lib.ddr_bmi_outputs_f32(4, *args[:10], None, 4, None), "null argument")
    assert lib.ddr_bmi_nexus_table(0, None, None, 4, None, None, None) == _lib.DDR_OK  # an empty dictionary


# ---- BmiInitConfig ----------------------------------------------------------------------------------------------
def test_init_config_defaults_and_validation():
    from pydantic import ValidationError

    cfg = BmiInitConfig(ddr_config="ddr.yaml", kan_checkpoint="kan.pt")
    assert cfg.device == "cpu" and cfg.timestep_seconds == 3600.0 and cfg.interpolation == "constant"
    assert cfg.hydrofabric_gpkg is None and cfg.conus_adjacency is None
    assert isinstance(cfg.ddr_config, Path) and isinstance(cfg.kan_checkpoint, Path)
    cfg = BmiInitConfig(ddr_config="ddr.yaml", kan_checkpoint="kan.pt", device="cuda:0", timestep_seconds=900.0,
                        interpolation="linear", hydrofabric_gpkg="hf.gpkg")
    assert (cfg.device, cfg.timestep_seconds, cfg.interpolation) == ("cuda:0", 900.0, "linear")
    assert cfg.hydrofabric_gpkg == Path("hf.gpkg")
    with pytest.raises(ValidationError):
        BmiInitConfig(ddr_config="ddr.yaml", kan_checkpoint="kan.pt", interpolation="cubic")
    with pytest.raises(ValidationError):
        BmiInitConfig(kan_checkpoint="kan.pt")


# ---- the tables -------------------------------------------------------------------------------------------------
VARS = {  # name: (units, type, itemsize)
    "land_surface_water_source__id": ("-", "int32", 4),
    "land_surface_water_source__volume_flow_rate": ("m3 s-1", "float64", 8),
    "ngen_dt": ("s", "int32", 4),
    "channel_water__id": ("-", "int64", 8),
    Q: ("m3 s-1", "float32", 4),
    "channel_water_flow__speed": ("m s-1", "float32", 4),
    "channel_water__mean_depth": ("m", "float32", 4),
}


def test_variable_tables_match_the_reference():
    b = DdrBmi()
    assert b.get_component_name() == "DDR-MuskingumCunge"
    assert b.get_input_var_names() == tuple(list(VARS)[:3]) and b.get_input_item_count() == 3
    assert b.get_output_var_names() == tuple(list(VARS)[3:]) and b.get_output_item_count() == 4
    for name, (units, typ, size) in VARS.items():
        assert b.get_var_units(name) == units, name
        assert b.get_var_type(name) == typ, name
        assert b.get_var_itemsize(name) == size, name
        assert b.get_var_location(name) == "node"
        assert b.get_var_grid(name) == 0
    assert b.get_var_units("anything_else") == "-" and b.get_var_type("anything_else") == "float64"
    with pytest.raises(NotImplementedError):
        b.get_var_nbytes(Q)


def test_time_and_grid_functions():
    b = DdrBmi()
    assert b.get_start_time() == 0.0 and b.get_end_time() == float("inf") and b.get_time_units() == "s"
    assert b.get_time_step() == 3600.0 and b.get_current_time() == 0.0
    assert b.get_grid_type(0) == "unstructured" and b.get_grid_rank(0) == 1
    assert b.get_grid_size(0) == 0 and b.get_grid_node_count(0) == 0
    assert b.get_grid_edge_count(0) == 0 and b.get_grid_face_count(0) == 0
    assert b.get_grid_shape(0, np.empty(1, np.int32))[0] == 0
    one = np.empty(1)
    for f in (b.get_grid_spacing, b.get_grid_origin, b.get_grid_x, b.get_grid_y, b.get_grid_z, b.get_grid_edge_nodes,
              b.get_grid_face_edges, b.get_grid_face_nodes, b.get_grid_nodes_per_face):
        with pytest.raises(NotImplementedError):
            f(0, one)


BMI_2_0 = """initialize update update_until finalize get_component_name get_input_item_count get_output_item_count
get_input_var_names get_output_var_names get_var_grid get_var_type get_var_units get_var_itemsize get_var_nbytes
get_var_location get_current_time get_start_time get_end_time get_time_units get_time_step get_value get_value_ptr
get_value_at_indices set_value set_value_at_indices get_grid_rank get_grid_size get_grid_type get_grid_shape
get_grid_spacing get_grid_origin get_grid_x get_grid_y get_grid_z get_grid_node_count get_grid_edge_count
get_grid_face_count get_grid_edge_nodes get_grid_face_edges get_grid_face_nodes get_grid_nodes_per_face""".split()


def test_method_set_is_bmi_2_0():
    assert len(BMI_2_0) == 41
    public = {k for k, v in vars(DdrBmi).items() if callable(v) and not k.startswith("_")}
    assert public - {"initialize_from", "dataset_factory"} == set(BMI_2_0)


# ---- before initialize ------------------------------------------------------------------------------------------
def test_before_initialize():
    b = DdrBmi()
    with pytest.raises(RuntimeError, match="not initialized"):
        b.update()
    with pytest.raises(RuntimeError, match="not initialized"):
        b.update_until(3600.0)
    for name in list(VARS)[3:]:
        assert isinstance(b.get_value_ptr(name), np.ndarray) and len(b.get_value_ptr(name)) == 0
    with pytest.raises(ValueError, match="Unknown output variable"):
        b.get_value_ptr("nonexistent_variable")
    with pytest.raises(ValueError, match="Unknown output variable"):
        b.get_value("land_surface_water_source__id", np.empty(1))
    b.set_value("nonexistent_variable", np.array([1.0]))  # BMI convention: ignored
    b.set_value("ngen_dt", np.array([900]))
    assert b._ngen_dt == 900
    b.finalize()
    with pytest.raises(RuntimeError, match="not initialized"):
        b.update()


def test_initialize_needs_a_dataset_factory_and_a_device(tmp_path):
    from types import SimpleNamespace

    import torch

    dc = SimpleNamespace(adjacency_matrix=torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DdrBmi().initialize_from(dc, {}, SimpleNamespace(), device="cpu")
    with pytest.raises(ValueError, match="interpolation"):
        DdrBmi().initialize_from(dc, {}, SimpleNamespace(), interpolation="cubic", device="cpu")
    ddr = tmp_path / "ddr.yaml"
    ddr.write_text("seed: 0\ndata_sources: {geospatial_fabric_gpkg: none.gpkg}\n")
    init = tmp_path / "bmi.yaml"
    init.write_text(f"ddr_config: {ddr}\nkan_checkpoint: {tmp_path / 'kan.pt'}\ndevice: cuda\n")
    with pytest.raises(RuntimeError, match="initialize_from"):
        DdrBmi().initialize(str(init))
    init.write_text(f"ddr_config: {ddr}\nkan_checkpoint: {tmp_path / 'kan.pt'}\n")  # device: cpu, the default
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DdrBmi().initialize(str(init))


# ---- the nexus mapping ------------------------------------------------------------------------------------------
def _gpkg(path, rows, table="flowpaths"):
    con = sqlite3.connect(str(path))
    con.execute(f"CREATE TABLE {table} (id TEXT, toid TEXT)")
    con.executemany(f"INSERT INTO {table} VALUES (?, ?)", rows)
    con.commit()
    con.close()
    return path


def test_nexus_mapping_cases(tmp_path):
    b = DdrBmi()
    b._num_segments = 3
    rows = [("wb-101", "nex-201"), ("wb-102", "nex-202"), ("wb-103", "nex-203"), ("wb-104", "tnx-9"),
            ("nex-5", "nex-6"), ("wb-999", "nex-777")]
    g = _gpkg(tmp_path / "a.gpkg", rows)
    assert b._build_nexus_mapping(g, ["cat-101", "cat-102", "cat-103"]) == {201: 0, 202: 1, 203: 2}
    # nexus and flowpath numbers need not agree; wb- divide ids work too
    g2 = _gpkg(tmp_path / "b.gpkg", [("wb-50", "nex-999"), ("wb-51", "nex-1000")])
    assert b._build_nexus_mapping(g2, np.array(["wb-51", "cat-50"])) == {999: 1, 1000: 0}
    # no flowpaths table: a segment's id is its nexus id
    g3 = _gpkg(tmp_path / "c.gpkg", [], table="other_table")
    assert b._build_nexus_mapping(g3, ["cat-10", "cat-20"]) == {10: 0, 20: 1}
    assert b._build_nexus_mapping(g3, None) == {0: 0, 1: 1, 2: 2}
    # no divide ids: segments are numbered 0..N-1, and only flowpaths with those numbers map
    assert b._build_nexus_mapping(g, None) == {}
    g4 = _gpkg(tmp_path / "d.gpkg", [("wb-2", "nex-30"), ("wb-0", "nex-10"), ("wb-7", "nex-70")])
    assert b._build_nexus_mapping(g4, None) == {30: 2, 10: 0}


# ---- update_until's bookkeeping ---------------------------------------------------------------------------------
def _reference_bookkeeping(current, time, dt):
    """ddr_bmi.py:264-272, 308 with the routing taken out."""
    remaining = time - current
    if remaining <= 0.0:
        return None
    n_steps = max(1, round(remaining / dt))
    executed = 0
    for _step in range(n_steps):
        if current >= time - 1e-6:
            break
        current += dt
        executed += 1
    return n_steps, executed, current


@pytest.mark.parametrize("dt", [900.0, 300.0, 3600.0, 0.1])
@pytest.mark.parametrize("start", [0.0, 3600.0, 1e7 + 0.3])
@pytest.mark.parametrize("ratio", [0.4, 1, 1.5, 2.5, 4, 8, 0.0, -1.0, 1e-9])
def test_step_count_and_time_bookkeeping(dt, start, ratio):
    time = start + ratio * dt
    want = _reference_bookkeeping(start, time, dt)
    got = plan_interval(start, time, dt)
    assert got == want
    if ratio <= 0:
        assert got is None
    elif start == 0.0 and ratio >= 0.4:
        n = {0.4: 1, 1: 1, 1.5: 2, 2.5: 2, 4: 4, 8: 8}[ratio]  # Python's round: halves go to the even count
        assert got[:2] == (n, n) and got[2] == sum([dt] * n, 0.0)


def test_target_within_the_time_tolerance_runs_no_step():
    # a target within 1e-6 s of now plans one step and runs none (the reference's time check)
    assert plan_interval(100.0, 100.0 + 5e-7, 900.0) == (1, 0, 100.0)
