"""The four host walks of scene_check.cpp (closest_host, nearest_host, multihit_host, count_visits) against tests/golden/host_walks.npz,
recorded by tests/golden/make_host_walks.py before their inner steps and their list were written once: on three host-built scenes, 64
points and 64 rays each, every output bit for bit and every counter to the unit. CPU only."""
import sys
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_host_walks as mk  # noqa: E402


@pytest.mark.parametrize("name", mk.SCENES)
def test_host_walks_equal_the_recorded_bits_and_counters(rtlib, name):
    """closest_host (brute force and walk, with and without radii), nearest_host and multihit_host (k = 1, 3, 8; brute force and walk;
    with and without a key; with and without a radius / tmax) and rt_scene_count_visits in modes 0, 1, 2 and 4: node_visits and
    tri_tests equal the recorded ones, every output array equals the recorded bits."""
    with np.load(GOLDEN / "host_walks.npz") as z:
        inp = {k: z[f"{name}/in/{k}"] for k in mk.INPUTS}
        bits, counters = z[f"{name}/bits"], z[f"{name}/counters"]
    s = mk.build(name, rtlib)
    try:
        res = mk.walks(s, inp)
    finally:
        s.close()
    at = c = 0
    for key, got in res.items():
        if mk.is_counter(key):
            assert int(got) == int(counters[c]), f"{name}: {key} is {int(got)}, recorded {int(counters[c])}"
            c += 1
        else:
            g = np.ascontiguousarray(got).view(np.uint32).reshape(-1)
            want = bits[at:at + g.size]
            bad = np.flatnonzero(g != want)
            assert g.size == want.size and bad.size == 0, f"{name}: {key} differs at {bad.size} of {g.size} words, first {bad[:1]}"
            at += g.size
    assert at == bits.size and c == counters.size
