"""GPU: every entry of include/vgx.h that takes a stream, driven from a non-blocking side stream behind a delay while the null stream
idles (the "sandwich" of tests/stream_order.py): the outputs must be those of the plain call, byte for byte, the entries the header
classes as asynchronous must return while the delay still runs, and three sensitivity rows show that the harness sees an entry that
ran on the wrong stream. One row per entry, each on a context of its own, on the smallest frame the entry's own test uses.

Every run prints, per row, the host time from the first enqueue of the sandwich to the entry's return and the calibrated delay
(STREAM_ORDER lines). Measured on an MI355X with a delay of 49.94 ms: 0.045 .. 0.194 ms for the asynchronous entries, at most 0.0039
of the delay; the entries that return data to the host take the delay, they wait for the side stream.
"""
import pytest

import stream_order as SO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    return SO.Env()


@pytest.fixture(scope="module")
def side(env):
    return SO.side_stream(env.torch)


@pytest.mark.parametrize("row", SO.CASES, ids=lambda r: r.name)
def test_entry_on_a_non_blocking_stream(env, side, row):
    SO.run_row(row, env, side)


@pytest.mark.parametrize("row", SO.SENSITIVITY, ids=lambda r: r.name)
def test_harness_sees_an_entry_on_the_wrong_stream(env, side, row):
    SO.run_row(row, env, side)
