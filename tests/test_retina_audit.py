"""The RetinaNet decision-margin audit's restatement (tests/_retina_audit_restatement.py) against the cases it was built for: each case
gives the margins it was designed to have, and each `wrong=` switch -- one rule replaced by a plausible wrong one -- changes the result of
at least one case.  tests/test_gpu_retina_audit.py then holds cald_op_retina_audit to the restatement bit for bit."""
import numpy as np
import pytest

import _retina_audit_restatement as A

F32 = np.float32
SMALL_CASES = sorted(k for k in A.CASES if k != "many")


@pytest.fixture(scope="module")
def exp(oracle):
    return oracle.exp_array


@pytest.mark.parametrize("name", SMALL_CASES)
def test_cases_give_the_margins_they_were_designed_to_have(exp, name):
    case = A.CASES[name]()
    s, b = case.inputs(exp)
    got = case.restate(exp)
    m = got["margins"]
    assert m.dtype == F32 and m.shape == (A.N_MARGINS,) and not np.isnan(m).any() and (m >= 0).all()
    assert np.isinf(m[[0, 1, 2, 3, 4, 5, 6, 12, 14]]).all()                      # RPN, RoI, argmax and cutout slots are not the tail's
    assert got["n"] == case.n, (name, got["n"])
    design = case.design(s, b)
    assert design, name
    for q, want in design.items():
        assert m[q] == F32(want), (name, q, m[q], want)


def test_the_designed_scores_are_where_the_cases_say(exp):
    """The cases speak of thr +- 3e-4, thr - 1e-4 and thr + 2e-3: the float32 sigmoids of their logits are that close to those."""
    s, _ = A.CASES["thr_other_class"]().inputs(exp)
    for got, want in ((s[1, 0], 0.05 + 3e-4), (s[2, 0], 0.05 - 3e-4), (s[3, 0], 0.05 - 1e-4), (s[3, 1], 0.05 - 1e-4), (s[4, 0], 0.05 + 2e-3)):
        assert abs(float(got) - want) < 2e-8
    m = A.CASES["thr_window"]().restate(exp)["margins"]
    assert abs(float(m[A.THR]) - 3e-4) < 1e-7
    assert abs(float(A.CASES["thr_other_class"]().restate(exp)["margins"][A.THR]) - 1e-4) < 1e-7


def direct_case():
    """Scores handed over directly, threshold 0: a score of exactly float32(1e-3) is a candidate at distance 1e-3 -- not INSIDE the window."""
    s = np.full((3, 2), -1.0, F32)                     # (handed over directly, the scores need not be sigmoids: far below the window)
    s[0, 0] = F32(1e-3); s[1, 1] = F32(0.5)
    b = np.array([[0, 0, 10, 10], [20, 20, 30, 30], [40, 40, 50, 50]], F32)
    return s, b


def test_the_window_is_open():
    s, b = direct_case()
    m = A.records(s, b, score_thr=0.0, per_class=5)["margins"]
    assert np.isinf(m[A.THR]) and m[A.IOU] == F32(0.5)
    assert A.records(s, b, score_thr=0.0, per_class=5, wrong="ge_window")["margins"][A.THR] == F32(1e-3)


@pytest.mark.parametrize("wrong", A.WRONG)
def test_every_wrong_rule_changes_some_case(exp, wrong):
    hit = []
    if wrong == "ge_window":
        s, b = direct_case()
        if A.records(s, b, score_thr=0.0, per_class=5)["margins"].tobytes() != A.records(s, b, score_thr=0.0, per_class=5, wrong=wrong)["margins"].tobytes():
            hit.append("direct")
    for name in SMALL_CASES:
        case = A.CASES[name]()
        right, bad = case.restate(exp), case.restate(exp, wrong=wrong)
        if right["margins"].tobytes() != bad["margins"].tobytes() or right["n"] != bad["n"]:
            hit.append(name)
    print(wrong, "->", hit)
    assert hit, wrong


def test_a_nan_score_is_no_candidate_and_in_no_window():
    s = np.full((2, 1), np.nan, F32)
    b = np.array([[0, 0, 10, 10], [20, 20, 30, 30]], F32)
    assert np.isinf(A.records(s, b)["margins"]).all()
