"""CPU, no library: the two decisions of the sparse convs answer what they answered on the commit before
SparseConvolution's pack fields became one cache and the window predicates one module -- the scripted drivers of
tests/pack_window_trace.py against tests/golden/pack_lifecycle_trace.json and window_decisions.json, written on that commit
by tests/golden/make_pack_window_traces.py."""
import json
import os

import pack_window_trace as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def test_pack_lifecycle_is_the_recorded_one(monkeypatch):
    """Every pack made -- layout, mode, into which buffer -- and every buffer handed out, in order: once-only use in training,
    packs made ahead consumed once, the cache per (version, pointer, device, layout) in eval, buffers reused across repacks
    and layout changes, adopted buffers, a data-gradient pack in the layout its forward decided on."""
    want = _golden("pack_lifecycle_trace.json")
    got = P.pack_lifecycle(monkeypatch)
    assert list(got) == list(want)
    for layer in want:
        for i, (a, b) in enumerate(zip(got[layer], want[layer])):
            assert a == b, (layer, i, a, b, got[layer][max(0, i - 4):i + 3], want[layer][max(0, i - 4):i + 3])
        assert len(got[layer]) == len(want[layer])
    log = want["5->16"]                            # the record itself: prepack() of the 5 -> 16 layer makes no dgrad pack ahead
    i = log.index(["step", "2 prepack: forward, dgrad, dgrad"])
    assert log[i + 1][:3] == ["pack", "generic", 0] and log[i + 2][0] == "get"


def test_window_decisions_are_the_recorded_ones(monkeypatch):
    """window_capable(), window_wgrad(), the prefetcher's (width, tables) hint and train.feature_stride for nine layers under
    four settings of the "subm_window" / "subm_window_wgrad" options."""
    want = _golden("window_decisions.json")
    got = json.loads(json.dumps(P.window_decisions(monkeypatch)))
    assert list(got) == list(P.OPTIONS) == list(want)
    for opt in want:
        for layer in want[opt]:
            assert got[opt][layer] == want[opt][layer], (opt, layer, got[opt][layer], want[opt][layer])
        assert list(got[opt]) == list(want[opt])
    d = want["23/6"]                               # the record itself, at the defaults
    assert [l for l in d if d[l]["window_capable"]] == ["5->16", "16->16", "32->32", "64->64", "16->32"]
    assert d["64->64"]["subm_hint bf16 grad"] == [64, True] and d["64->64"]["subm_hint bf16 no_grad"] == [64, False]
    assert d["16->16"]["subm_hint bf16 grad"] == d["16->16"]["subm_hint bf16 no_grad"] == [16, False]
    assert d["128->128"]["subm_hint bf16 grad"] == [None, True]
    assert (d["5->16"]["feature_stride yxz"], d["5->16"]["feature_stride zyx"]) == (16, None)
    assert want["7/6"]["5->16"]["feature_stride yxz"] is None
