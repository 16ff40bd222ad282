"""Host-side checks of the long-slate attention feature (no GPU): the S = 1000 reference golden against the oracle, and the C ABI /
binding / Python limit of the key-tiled entries."""
import json
import os
import re

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _golden_long():
    with open(os.path.join(HERE, "golden", "manifest_r5.json")) as f:
        case = json.load(f)["encoder_long"][0]
    return case, np.load(os.path.join(HERE, "golden", "encoder_long.npz"), allow_pickle=False)


def test_long_slate_golden_matches_the_oracle():
    """tests/golden/encoder_long.npz (the reference at S = 1000, eval mode) reproduced by the oracle in fp32 (same arithmetic as the
    reference) at the bar make_golden_r5.py pinned it with."""
    import ltr_encoder_oracle as EO
    import ltr_oracle as O
    case, g = _golden_long()
    cid = case["id"]
    assert case["S"] == 1000 and case["S"] > 512
    x, y, mask = (torch.from_numpy(g[f"{cid}/{n}"]) for n in ("x", "y", "mask"))
    assert tuple(x.shape) == (case["B"], case["S"], case["n_features"]) and bool(mask.any())
    sd = {k: torch.from_numpy(g[f"{cid}/w/{k}"]) for k in case["keys"]}
    cfg = EO.config_of(dict(fc_model=case["fc_model"], transformer=case["transformer"]), case["n_features"])
    s, l, grads = EO.scores_and_grads(sd, x, mask, cfg, lambda s_: O.approx_ndcg(s_, y.to(s_.dtype)), dtype=torch.float32)
    want_s = torch.from_numpy(g[f"{cid}/scores"])
    assert float((s - want_s).abs().max()) <= 2e-5 * float(want_s.abs().max())
    assert abs(float(l) - float(g[f"{cid}/loss"])) <= 2e-5 * abs(float(g[f"{cid}/loss"]))
    ref = {k: torch.from_numpy(g[f"{cid}/g/{k}"]) for k in case["keys"]}
    floor = 1e-3 * max(float(v.abs().max()) for v in ref.values())
    for k, want in ref.items():
        e = float((grads[k] - want).abs().max()) / max(float(want.abs().max()), floor)
        assert e <= 2e-5, (k, e)


def test_tiled_entries_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "ltr_encoder.h")) as f:
        header = f.read()
    from ltr_mi355x._lib import _PROTOTYPES
    for name in ("ltr_enc_attention_fwd_tiled", "ltr_enc_attention_bwd_tiled"):
        assert re.search(r"\bint\s+" + name + r"\(", header), name
        assert name in _PROTOTYPES, name
    assert "2048" in header


def test_python_slate_limit_is_2048():
    from ltr_mi355x import encoder
    assert encoder.MAX_ATTN_SLATE == 2048
