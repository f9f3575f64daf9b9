"""The context's view-bound state against the recording of the library before
csrc/rt_view.h (tests/view_trace.py): the same seeded call sequences leave the
same statuses, refusals, temporal and filter images, adaptive statistics,
assembled-frame reports and frame counters after every call — CPU backend, no
GPU needed.
"""
import json

import pytest

import view_trace as T
from test_lifecycle_trace import first_difference


@pytest.fixture(scope="module")
def golden():
    with open(T.GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("threads", [1, 5])
def test_trace_equals_the_recording(bwrt_lib, golden, threads):
    got = T.traces(bwrt_lib, threads=threads)
    assert got == golden, first_difference(got, golden)


def check_coverage(cov):
    """What a recording has to contain to be worth comparing with."""
    assert set(cov["ok"]) == {name for name, _ in T.WEIGHTS}
    assert min(cov["ok"].values()) >= 5, cov["ok"]
    assert cov["promotions"] >= 10
    # histories dropped by a scene change, a shape change through rt_init_rand and
    # through a render of the other shape, and rt_temporal_reset: the next temporal
    # call returns the length 1 everywhere (the second figure; the first also
    # counts the calls that found no history in a frame of more than one sample,
    # whose length is that count everywhere: view_trace's docstring)
    assert min(cov["drops"].values()) >= 3, cov["drops"]
    assert min(cov["drops_length_1"].values()) >= 3, cov["drops_length_1"]
    refused = cov["refused"]
    assert refused[("adaptive_reprojected", "no pending temporal set")] >= 3
    assert refused[("adaptive_reprojected", "has no moments")] >= 3
    assert cov["ok"]["adaptive_reprojected"] >= 5
    assert cov["var_on_plain_history"] >= 3  # rt_temporal_var on a history without moments
    assert cov["plain_on_var_history"] >= 3
    # a shard context: filters on a current assembled frame, a stale one, none
    assert cov["shard_filter_ok"] >= 5 and cov["shard_filter_ok_counted"] >= 2
    assert cov["shard_filter_refused"]["is stale"] >= 3
    assert cov["shard_filter_refused"]["row shard"] >= 3
    assert cov["assembled"] == [0, 1]
    assert set(cov["assembled_lost_after"]) >= {"set_scene", "set_camera", "controls_moved", "reshape",
                                                "assemble_drop"}


def test_the_recording_covers_the_views(golden):
    check_coverage(T.coverage(golden))
