"""gpmpc_knn_plan without a GPU: the part count and the queries per wave of every shape the
device tests (tests/test_gpu_knn.py, tests/test_gpu_terminal.py) say they cover, the split
rule over a sweep of shapes, the refusals, and the constants the binding repeats."""
import os
import re

import numpy as np
import pytest

from conftest import golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def L():
    from gp_mpc_rocket_landing_amd import _lib
    return _lib


def test_binding_constants_match_the_kernels():
    src = open(os.path.join(REPO, "gp_mpc_rocket_landing_amd", "csrc", "knn.hip")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (KNN_\w+) (\d+)", src)}
    lib = L()
    for k in ("KNN_MAXD", "KNN_MAXK", "KNN_Q", "KNN_PART_ROWS", "KNN_MAX_PARTS", "KNN_TARGET_WG"):
        assert val[k] == getattr(lib, k), k
    assert val["KNN_THREADS"] == 256 == 4 * val["KNN_MAXK"] and val["KNN_WAVES"] == 4
    for name in ("gpmpc_knn_create", "gpmpc_knn_destroy", "gpmpc_knn_query", "gpmpc_knn_interp", "gpmpc_knn_plan"):
        assert name in lib.EXPORTED
    assert lib.abi_version() == 4


def test_the_shapes_of_the_device_tests():
    import test_gpu_knn as t
    lib = L()
    q = lib.KNN_Q
    assert t._batches() == [1, q - 1, q, q + 1, 70]
    for B in t._batches():
        for n in t.NS:
            parts, qw = lib.knn_plan(n, 7, B)
            assert qw == (1 if B == 1 else q), (n, B)
            # no split up to 1024 rows, two parts from 1025 (768 + 257), three at 2049 (768 + 768 + 513)
            assert parts == (1 if n <= 1024 else 2 if n <= 2048 else 3), (n, B, parts)
    assert {1024, 1025, 2048, 2049} <= set(t.NS)
    # the merge of many parts: the most the plan makes, and an odd count
    assert [lib.knn_plan(n, d, B)[0] for n, d in t.BIG for B in (1, 3)] == [64, 64, 33, 33]
    assert lib.KNN_MAX_PARTS == 64
    # the pattern tests: single-part and split sets
    for n, parts in ((700, 1), (2049, 3), (300, 1), (1300, 2), (257, 1), (1100, 2), (1500, 2)):
        assert lib.knn_plan(n, 7, 5)[0] == parts == lib.knn_plan(n, 7, 1)[0], n
    # the fixture's sets (tests/test_gpu_terminal.py): one part, a full wave of queries for the batches
    g = golden("safeset.npz")
    for name in ("s7", "s14"):
        n = len(g[f"{name}_q"])
        assert lib.knn_plan(n, int(name[1:]), len(g[f"{name}_Xq"])) == (1, q)
        assert lib.knn_plan(n, int(name[1:]), 1) == (1, 1)


def test_the_split_rule():
    lib = L()
    for n in (1, 1000, 1024, 1025, 4096, 5000, 65536, 131072, 10 ** 6, 2 ** 31 - 1):
        for B in (1, 2, 4, 64, 257, 1024, 10 ** 5):
            parts, qw = lib.knn_plan(n, 7, B)
            groups = -(-B // qw)
            want = min(-(-lib.KNN_TARGET_WG // groups), -(-n // lib.KNN_PART_ROWS), lib.KNN_MAX_PARTS)
            length = -(-(-(-n // want)) // 256) * 256           # a multiple of the workgroup's stride
            assert parts == -(-n // length) <= want, (n, B)
            assert (parts - 1) * length < n <= parts * length   # every part has rows, together all of them
    # the probe's shapes (docs/PERF_HISTORY.md)
    assert [lib.knn_plan(131072, 7, B) for B in (1, 64, 1024)] == [(64, 1), (16, 2), (1, 2)]
    assert [lib.knn_plan(65536, 14, B) for B in (1, 64, 1024)] == [(64, 1), (16, 2), (1, 2)]
    assert lib.knn_plan(300, 1, 1, 1) == lib.knn_plan(300, 32, 1, 64) == (1, 1)     # d and k do not move the plan


@pytest.mark.parametrize("args", [(0, 7, 1, 4), (10, 0, 1, 4), (10, 33, 1, 4), (10, 7, 0, 4), (10, 7, 1, 0),
                                  (10, 7, 1, 65)])
def test_refusals(args):
    lib = L()
    with pytest.raises(lib.HIPError) as e:
        lib.knn_plan(*args)
    assert e.value.rc == -2 and "bad argument" in str(e.value)


def test_binding_refuses_before_any_device_call():
    lib = L()

    class NoCtx:
        h = None

    bad = np.ones((4, 3)); bad[2, 1] = np.inf
    with pytest.raises(ValueError):
        lib.KnnSet(NoCtx, bad)
    with pytest.raises(ValueError):
        lib.KnnSet(NoCtx, np.ones((4, 3)), q=np.array([0.0, np.nan, 0.0, 0.0]))
    with pytest.raises(ValueError):
        lib.KnnSet(NoCtx, np.ones((4, 3)), fuel_req=np.ones(3))
