"""The context's lifecycle against the recording of the library before
csrc/rt_accum.h (tests/lifecycle_trace.py): the same seeded call sequences
leave the same frame counter, tracking state, counts, pixel state, variance,
filter images and statistics after every call — CPU backend, no GPU needed.
"""
import json

import pytest

import lifecycle_trace as T


@pytest.fixture(scope="module")
def golden():
    with open(T.GOLDEN) as f:
        return json.load(f)


def first_difference(got, want):
    for seed in want:
        for i, (a, b) in enumerate(zip(got[seed], want[seed])):
            if a != b:
                return f"seed {seed} step {i}: got {a}, recorded {b}"
    return None


@pytest.mark.parametrize("threads", [1, 5])
def test_trace_equals_the_recording(bwrt_lib, golden, threads):
    got = T.traces(bwrt_lib, threads=threads)
    assert got == golden, first_difference(got, golden)


def test_the_recording_covers_the_lifecycle(golden):
    """What the committed recording has to contain to be worth comparing with."""
    cov = T.coverage(golden)
    assert set(cov["ok"]) == {name for name, _ in T.WEIGHTS}
    assert min(cov["ok"].values()) >= 5, cov["ok"]
    assert cov["unequal"] >= 0.10 * cov["records"]
    refused = cov["refused"]
    assert refused[("render", "non-uniform")] >= 3  # a uniform render that would continue
    for name in ("denoise", "denoise_var", "temporal"):  # the switch off
        assert refused[(name, "non-uniform")] >= 3, name
    assert sum(n for (_, why), n in refused.items() if why == "no frame accumulated yet") >= 3
    assert refused[("adaptive", "not live")] >= 3
    assert cov["drops"] >= 3  # tracking ended by a first_frame that is not the next one
