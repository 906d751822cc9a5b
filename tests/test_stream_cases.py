"""The case table of tests/stream_cases.py, checked on the CPU: every entry point of the ABI is either
replayed by tests/test_streams_gpu.py or excluded with a reason, and the two data sets of every case
really differ.  A new entry point fails here until it gets a case."""
import torch

import stream_cases as sc
from mpi_vision_amd import _lib


def test_every_entry_point_is_covered_or_excluded():
    assert sc.COVERED | set(sc.EXCLUDED) == set(_lib._SIGS)
    assert not sc.COVERED & set(sc.EXCLUDED)
    assert all(sc.EXCLUDED.values()), "every exclusion carries its reason"
    assert "mpiv_render_packed_census" in sc.COVERED


def test_every_covered_entry_point_has_a_case():
    called = {e for c in sc.CASES for e in c.entries}
    assert called <= set(_lib._SIGS)
    assert sc.COVERED - called == set(), "entry points without a replay case"
    assert len(set(sc.CASE_IDS)) == len(sc.CASE_IDS), "case names are the test ids: unique"


def test_both_data_sets_differ_in_every_input_buffer():
    for c in sc.CASES:
        a, b = c.inputs(0), c.inputs(1)
        assert a.keys() == b.keys(), c.name
        for n in a:
            assert a[n].shape == b[n].shape and a[n].dtype == b[n].dtype and a[n].stride() == b[n].stride(), \
                f"{c.name}: {n} changes shape, type or layout between the data sets"
            assert not torch.equal(a[n], b[n]), f"{c.name}: {n} is the same in both data sets"
        assert not set(a) & set(c.outputs) and not set(c.state) & (set(a) | set(c.outputs)), c.name


def test_listed_shapes_reach_distinct_kernels():
    """The shapes of one entry are there for its production routes: where mpiv_route knows the entry, the
    listed shapes dispatch to that many different kernels (template arguments included)."""
    V = sc.VP
    for entry in ("render_packed", "render_packed_ct", "render_packed_u8", "render_packed_f16"):
        names = {_lib.route(entry, H, W, P, V)[0] for H, W, P in sc.PACKED_SHAPES}
        assert len(names) == len(sc.PACKED_SHAPES), f"{entry}: {names}"
    names = {_lib.route("plane_sweep", sc.SB, sc.SHS, sc.SWS, C, D, sc.SHT, sc.SWT)[0] for C, D in sc.SWEEP_CD}
    assert len(names) >= 4, f"plane_sweep: direct, pixel per lane, depth lanes and generic: {names}"
    assert "chunk" in _lib.route("render", sc.NB, sc.NH, sc.NW, 11)[0]
