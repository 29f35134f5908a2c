"""Convolution kernel selection, pinned: the host-only query entry points must answer every problem of the census grid exactly as
recorded in tests/golden/conv_selection.npz (tests/golden/make_conv_selection.py wrote it and regenerates the problem table).
Pure host code: no GPU needed."""
import importlib.util
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_conv_selection", os.path.join(GOLD, "make_conv_selection.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_conv_selection_census():
    gen = _generator()
    gold = np.load(os.path.join(GOLD, "conv_selection.npz"))
    P = gen.problems()
    assert gen.digest(P) == str(gold["problems_sha256"]), "the problem table changed: the recorded answers belong to another grid"
    assert os.path.getsize(os.path.join(GOLD, "conv_selection.npz")) < 500_000
    ans = gen.ask(P)
    for name in gen.ANSWERS:
        if name == "partials_rows" and gen.cu_count() != int(gold["cu_count"]):
            continue          # 8 rows per conv_k3 workgroup, one workgroup per CU: comparable on the recorded CU count only
        bad = np.nonzero(ans[name] != gold[name])[0]
        assert bad.size == 0, (f"{name}: {bad.size} of {len(P)} answers differ, first: " +
                               "; ".join(f"{dict(zip(gen.COLS, P[i].tolist()))} -> {int(ans[name][i])}, recorded {int(gold[name][i])}" for i in bad[:3]))
