"""The specification side of tests/transform_extremes.py, without a GPU: every family x matrix meets the conditions it is named for
(zero-direction segments, exact collinear joins and hairpins, joins either side of the |cross| = 0.01 threshold, lenSqr beyond 2^100 and
at +inf), the reference's answer to it is finite and within the 65 536-vertex mesh limit, and the restatement (kind="port") gives the same
bytes. When a case of tests/test_gpu_transform_extremes.py fails while this file is green, the specification is settled and the kernel
is what is wrong. A case whose conditions do not hold FAILS: nothing here skips."""
import numpy as np
import pytest

import transform_extremes as tx
from util import bytes_equal

CASES = tx.all_cases()


@pytest.fixture(scope="module")
def ref_kind(oracle):
    assert oracle.available("reference"), "oracle/_ref/libvgref.so (the reference compiled from its own sources) is what these cases are pinned on"
    return "reference"


@pytest.mark.parametrize("c", CASES, ids=tx.case_id)
def test_case_meets_the_conditions_it_is_named_for(ref_kind, c):
    ref = tx.reference(*c)
    tot = tx.check_case(c, ref)
    print(tx.case_id(c), {k: v for k, v in tot.items() if v})


@pytest.mark.parametrize("c", CASES, ids=tx.case_id)
def test_reference_output_is_finite_and_within_the_mesh_limit(ref_kind, c):
    ref = tx.reference(*c)
    assert ref.pos.shape[0] > 0 and ref.meshes.shape[0] > 0
    assert np.isfinite(ref.pos).all(), np.flatnonzero(~np.isfinite(ref.pos).all(axis=1))[:5]
    assert np.isfinite(ref.poly).all()
    assert int(ref.meshes["num_vertices"].max()) <= tx.MESH_VERTEX_LIMIT
    # (what the GPU file's largest inputs are sized by: ~60 k vertices for fuzz, a 40-instance batch for closed)
    if c[0] == "fuzz":
        assert ref.pos.shape[0] < 65000


@pytest.mark.parametrize("c", CASES, ids=tx.case_id)
def test_restatement_equals_the_reference_in_every_byte(ref_kind, oracle, c):
    ref = tx.reference(*c)
    ps, d = tx.case(*c)
    port = oracle.tessellate(ps, d, kind="port", want_flat=True)
    assert port.sizes == ref.sizes
    for k in ("pos", "color", "idx", "meshes", "poly", "subpaths", "draw_info"):
        assert bytes_equal(getattr(port, k), getattr(ref, k)), (tx.case_id(c), k)


def test_closed_extreme_draws_differ_from_the_counted_ones_in_the_matrix_alone():
    for kind, (ninst, _) in tx.CLOSED.items():
        ps, d, e = tx.closed_case(kind)
        assert d.shape[0] == ninst * ps.npaths > 2048
        for f in d.dtype.names:
            assert (f == "mtx") != np.array_equal(d[f], e[f]), f


def test_walk_meshes_are_all_long_strokes():
    """k_stroke_long takes batches whose stroke meshes all have >= 128 elements (VGX_LONG_STROKE) and no other mesh kind."""
    ref = tx.reference("walks", "identity")
    assert int(ref.subpaths["num_vertices"].min()) >= 128
    kinds = ref.meshes["subpath_kind"] >> 28
    assert np.isin(kinds, (tx.capi.MESH_STROKE, tx.capi.MESH_STROKE_AA)).all()


def test_classifier_on_hand_computed_joins():
    """The checker itself, on polylines whose classes are known by hand."""
    class Flat:
        pass
    f = Flat()
    f.poly = np.array([[0, 0], [10, 0], [20, 0], [3, 0], [3, 8],      # collinear, hairpin, turn
                       [0, 0], [1, 0], [1.003, 0.0005], [5, 5],        # a zero-direction segment (9e-6 + 2.5e-7 < 1e-5) between two ordinary ones
                       [0, 0], [2e15, 0], [2e15, 1e20]], dtype=np.float32)  # 4e30 > 2^100, 1e40 = +inf
    f.subpaths = np.zeros(3, dtype=tx.capi.subpath_dtype)
    f.subpaths["first_vertex"] = [0, 5, 9]
    f.subpaths["num_vertices"] = [5, 4, 3]
    f.subpaths["flags"] = [0, 0, 1]
    f.draw_info = np.zeros(3, dtype=tx.capi.draw_info_dtype)
    f.draw_info["num_subpaths"] = 1
    c = tx.classify(f, 3)
    assert c["segments"].tolist() == [4, 3, 3] and c["joins"].tolist() == [3, 2, 3]
    assert (c["collinear"][0], c["hairpin"][0], c["turn"][0]) == (1, 1, 1)
    assert c["zero_dir"].tolist() == [0, 1, 0]
    assert c["huge"].tolist() == [0, 0, 1] and c["inf"].tolist() == [0, 0, 2]
