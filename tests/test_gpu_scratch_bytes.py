"""GPU: vgx_scratch_bytes counts every buffer the context owns (the owner list of csrc/vgx_scratch.h), and the list is the
context's own."""
import importlib

import pytest

pytestmark = pytest.mark.gpu


def test_scratch_bytes_counts_the_partition_table_and_is_per_context(wl):
    rt = importlib.import_module("vg-renderer_amd.runtime")
    ctx = rt.Context(0)
    ps, draws = wl.tiger(1)
    pset = rt.PathSet(ctx, ps)
    dd = rt.upload_draws(draws)
    n = draws.shape[0]
    rt.partition(ctx, pset, dd, n, 2)
    small = ctx.scratch_bytes()
    bounds, weights = rt.partition(ctx, pset, dd, n, 65536)
    large = ctx.scratch_bytes()
    assert bounds[0] == 0 and bounds[-1] == n and len(weights) == 65536
    # every other buffer of the call is sized by the draws, which did not change: the difference is the table of the call
    # ([nparts + 1] bounds + weights, 8 bytes each)
    assert large - small >= (65536 + 1) * 2 * 8, (small, large)
    pset.close()
    ctx.close()
    other = rt.Context(0)
    try:
        assert other.scratch_bytes() < large, (other.scratch_bytes(), large)
    finally:
        other.close()
