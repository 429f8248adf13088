"""The committed fixtures must stay in step with the recipe: every fixture the generators under tests/golden/ write (make_golden*.py,
run where the reference tree is present) is committed, and no other -- the same case lists as tests/cases.py, and every parity case
with its recorded oracle-vs-reference agreement.  (Round 1 shipped a make_golden.py that crashed at HEAD without any test noticing.)"""
import json
import os

import cases as C
import golden_util as G


def test_case_lists_match_cases_py():
    made = {f[:-4] for f in os.listdir(G.GOLDEN_DIR) if f.endswith(".npz")}
    want = (set(C.OP_CASES) | set(C.E2E_CASES) | {c + "_metrics" for c in C.E2E_CASES} | {"dataset_ops", "rollout_ops"} | set(C.TRAIN_FIXTURES)
            | {"pointnet_util_host"})
    assert made == want, (made ^ want)
    rep = json.load(open(os.path.join(G.GOLDEN_DIR, "oracle_vs_reference.json")))
    assert set(C.OP_CASES) | set(C.E2E_CASES) <= set(rep)
