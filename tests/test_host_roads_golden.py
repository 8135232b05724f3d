"""CPU test of the host side of the indexed device calls against tests/golden/host_roads.json, the record
tests/golden/make_host_roads.py made of the library before the host roads were gathered into shared pieces: every scratch and
output size on the layouts' edges, every refusal with its code and text (and, through the calls that trip two at once, the order
in which a call's arguments are judged), every *_status of a null scratch.  No GPU: the recorded calls pass made-up integers as
device pointers and a scratch that is too small, so none of them gets as far as a launch."""
import importlib
import itertools
import json
import os

import pytest

from tests.golden import make_host_roads as gen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_roads.json")


@pytest.fixture(scope="module")
def lib():
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.build()
    return pkg.lib()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_record_covers_what_the_generator_lists(golden):
    assert set(golden["sizes"]) == set(gen.SIZES)
    assert set(golden["refusals"]) == set(gen.REFUSALS)
    assert set(golden["statuses"]) == set(gen.STATUSES)
    for name, spec in gen.REFUSALS.items():
        assert len(golden["refusals"][name]) == len(gen.refusal_calls(spec)), name


def test_sizes(lib, golden):
    for name, rec in golden["sizes"].items():
        fn = getattr(lib, name)
        axes = [[tuple(v) if isinstance(v, list) else v for v in axis] for axis in rec["axes"]]
        points = list(itertools.product(*axes))
        assert len(points) == len(rec["values"]), name
        for point, want in zip(points, rec["values"]):
            assert int(fn(*gen.flat(point))) == want, (name, point)


def test_sizes_checked_by_hand(lib):
    assert lib.wah_splice_scratch_bytes(992 * 4, 3, 2) == 1792
    assert lib.wah_from_positions_scratch_bytes(992 * 4097, 5) == 1536
    assert lib.wah_select_scratch_bytes(992 * 4097, 1) == 34560
    assert lib.wah_bsi_kth_grouped_scratch_bytes(992, 20, 7, 3) == 17408
    assert lib.wah_fetch_scratch_bytes(992 * 3, 1000) == 1280


def test_refusals(lib, golden):
    for name, calls in golden["refusals"].items():
        fn = getattr(lib, name)
        for call in calls:
            assert call["rc"] in (gen.WAH_ERR_ARG, gen.WAH_ERR_WORKSPACE), (name, call)  # (the record holds no call that runs)
            keep = [gen.native(a) for a in call["args"]]
            rc = int(fn(*keep))
            assert (rc, lib.wah_last_error().decode()) == (call["rc"], call["error"]), (name, call["args"])


def test_statuses(lib, golden):
    for name, rec in golden["statuses"].items():
        assert rec["rc"] == gen.WAH_ERR_ARG
        assert int(getattr(lib, name)(*rec["args"])) == rec["rc"], name
