"""CPU: the yardstick of match by projection (project_match_ref.py) on the shared cases (project_match_cases.py): the hand-worked case, every status
code, the margin guard that keeps the device's rounding out of every answer, and a sensitivity guard per rule."""
import numpy as np
import pytest

import project_match_cases as PC
import project_match_ref as R


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in PC.all_cases()}


@pytest.fixture(scope="module")
def answers(cases):
    out = {}
    for name, c in cases.items():
        margins = []
        out[name] = (PC.reference(c, margins=margins), margins)
    return out


def test_case_names_are_unique():
    names = [c["name"] for c in PC.all_cases()]
    assert len(names) == len(set(names))


def test_hand_worked_case(answers):
    got, _ = answers["hand_worked"]
    for key, want in PC.HAND_WORKED_ANSWER.items():
        assert got[key].tolist() == want, key


def test_every_status_is_reached(answers):
    got, _ = answers["every_status"]
    assert got["status"].tolist() == [R.MATCHED, R.CONTESTED, R.TOO_FAR, R.AMBIGUOUS, R.NO_CANDIDATE, R.BEHIND, R.BEHIND, R.OUTSIDE, R.INVALID, R.INVALID, R.MATCHED]
    assert got["match"].tolist() == [0, -1, -1, -1, -1, -1, -1, -1, -1, -1, 2]
    assert got["dist"].tolist() == [5, 9, 70, 10, -1, -1, -1, -1, -1, -1, 0]
    assert got["n_cand"].tolist() == [1, 1, 1, 2, 0, 0, 0, 0, 0, 0, 2]
    seen = set()
    for got, _ in answers.values():
        seen |= set(got["status"].tolist())
    assert seen == set(range(8))


def test_generated_cases_decide_something(answers):
    """the larger generated cases reach every code an honest input can (all but INVALID), so a parity failure there has something to show"""
    for name in ("kitti", "random_8x700x900"):
        assert set(answers[name][0]["status"].tolist()) >= set(range(7)), name


def test_margin_guard(cases, answers):
    """no quantity compared in steps 1-3 (Pz against the gates, u and v against the borders, |x_j - u| - r) lies within 1e-6 of its bound"""
    for name, (_, margins) in answers.items():
        finite = [m for m in margins if m == m]
        assert not finite or min(finite) >= 1e-6, (name, min(finite))
    for c, _ in PC.invalid_cases():
        margins = []
        PC.reference(c, margins=margins)
        assert min(m for m in margins if m == m) >= 1e-6, c["name"]


def test_invalid_cases_mark_exactly_the_affected_landmarks():
    for c, bad in PC.invalid_cases():
        L = len(c["lm_desc_row"])
        got = PC.reference(c, out=PC.sentinel_out(L))
        is_bad = got["status"] == R.INVALID
        assert np.flatnonzero(is_bad).tolist() == bad, c["name"]
        assert (got["match"][is_bad] == -1).all() and (got["dist"][is_bad] == -1).all()
        untouched = got["status"] == PC.FILL
        assert (got["match"][untouched] == PC.FILL).all()
        assert not untouched.any(), c["name"]


def test_two_items_on_one_image_do_not_contest(cases):
    c = cases["two_items_one_image"]
    whole = PC.reference(c)
    for m in range(2):
        lo, hi = c["lm_off"][m], c["lm_off"][m + 1]
        alone = dict(c, lm_off=np.array([0, hi - lo], np.int32), item_img=c["item_img"][m:m + 1], item_T=c["item_T"][m:m + 1], lm_xyz=c["lm_xyz"][lo:hi],
                     lm_desc_row=c["lm_desc_row"][lo:hi])
        got = PC.reference(alone)
        for key in got:
            assert np.array_equal(got[key], whole[key][lo:hi]), (m, key)


@pytest.mark.parametrize("rule, name, override", [("radius", "lm65", dict(radius_px=0.5)), ("tau", "lm65", dict(tau=40)), ("ratio", "ratio_on", dict(ratio_pct=0)),
                                                   ("depth gate", "lm65", dict(z_max=1e4))])
def test_each_rule_changes_an_answer(cases, answers, rule, name, override):
    base = answers[name][0]
    other = PC.reference(cases[name], **override)
    assert not np.array_equal(base["status"], other["status"]), rule


def test_the_mutual_step_changes_an_answer(answers):
    """without step 5 a CONTESTED landmark would have kept its keypoint"""
    for name in ("lm65", "claimed_by_300"):
        assert (answers[name][0]["status"] == R.CONTESTED).any(), name
    got = answers["claimed_by_300"][0]
    assert got["status"][0] == R.MATCHED and got["match"][0] == 1 and (got["status"][1:] == R.CONTESTED).all() and (got["dist"] == 7).all()


def test_duplicate_descriptors_go_to_the_smaller_keypoint(cases, answers):
    got = answers["duplicate_descriptors"][0]
    assert got["status"].tolist() == [R.MATCHED, R.MATCHED] and got["match"].tolist() == [0, 5] and got["n_cand"].tolist() == [5, 1]
    assert PC.reference(cases["duplicate_descriptors"], ratio_pct=80)["status"].tolist() == [R.AMBIGUOUS, R.MATCHED]
