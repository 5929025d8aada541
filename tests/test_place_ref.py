"""CPU: tests/place_ref.py -- the yardstick of the place database's GPU tests -- checked by hand: a 3-entry database whose scores are worked out
in the comments, the tau boundary, the gap boundary, the tie order of the selection, K above the number of eligible entries, and the add rules."""
import numpy as np

import place_ref as P


def _row(*bits):
    """a 32-byte descriptor with exactly the given bit positions (0..255) set"""
    d = np.zeros(32, np.uint8)
    for b in bits:
        d[b // 8] |= np.uint8(1 << (b % 8))
    return d


def _db():
    """entry 0 (frame 0): rows a = {}, b = {0..9}            (10 bits)
       entry 1 (frame 5): rows a' = {200}, c = {0..9, 100..104} (15 bits), d = {0..255 step 2} (128 bits)
       entry 2 (frame 9): rows b' = {0..9, 50} (11 bits), a = {}
    hamming: a-a' 1, a-c 15, a-d 128, b-a' 11, b-c 5, b-d 10 + 128 - 2 * 5 = 128 (d holds the even bits: 0, 2, 4, 6, 8 of b's ten);
             b'-a 11, b'-b 1, a-a 0, a-b 10"""
    a, b = _row(), _row(*range(10))
    a1, c, d = _row(200), _row(*range(10), *range(100, 105)), _row(*range(0, 256, 2))
    b1 = _row(*range(10), 50)
    db = P.PlaceRef(rows=4, capacity=8)
    assert db.add([np.stack([a, b]), np.stack([a1, c, d]), np.stack([b1, a])], [2, 3, 2], [0, 0, 0], [0, 5, 9]) == 0
    return db


def test_hamming_table_by_hand():
    db = _db()
    assert np.array_equal(P.hamming_table(db.desc[0], db.desc[1]), [[1, 15, 128], [11, 5, 128]])
    assert np.array_equal(P.hamming_table(db.desc[2], db.desc[0]), [[11, 1], [0, 10]])


def test_three_entry_scores_by_hand():
    db = _db()
    # query 2 (frame 9), min_gap 1: entries 0 and 1 are eligible, itself is not.
    #   against 0: row b' -> min(11, 1) = 1, row a -> min(0, 10) = 0: both <= 4 -> 2
    #   against 1: row b' -> min(b'-a' 12, b'-c 6, b'-d 11 + 128 - 2 * 5 = 129) = 6; row a -> min(1, 15, 128) = 1 -> only a at tau 4 -> 1
    s = db.score(0, 3, tau=4, min_gap=1)
    assert np.array_equal(s[2], [2, 1, -1])
    # query 1 (frame 5) against 0: a' -> min(1, 11) = 1; c -> min(15, 5) = 5; d -> 128: tau 4 -> 1
    assert np.array_equal(s[1], [1, -1, -1])
    assert np.array_equal(s[0], [-1, -1, -1])
    # the score is asymmetric: entry 0's rows against entry 1 at tau 4: a -> 1 (hit), b -> 5 (miss) = 1; at tau 5 both = 2, while 1 against 0 at tau 5 = 2 (a', c)
    assert P.score_pair(db.desc[0], db.desc[1], 4) == 1 and P.score_pair(db.desc[0], db.desc[1], 5) == 2
    assert P.score_pair(db.desc[1], db.desc[0], 5) == 2 and P.score_pair(db.desc[1], db.desc[0], 200) == 3


def test_tau_boundary():
    db = _db()
    # row c of entry 1 is at distance exactly 5 from its nearest row of entry 0
    assert db.score(1, 1, tau=4, min_gap=1)[0, 0] == 1 and db.score(1, 1, tau=5, min_gap=1)[0, 0] == 2
    # tau 0 counts exact duplicates only (row a of entry 2 equals row a of entry 0); tau 255 counts every row of a non-empty pair
    assert db.score(2, 1, tau=0, min_gap=1)[0, 0] == 1 and db.score(2, 1, tau=255, min_gap=1)[0, 1] == 2
    assert P.score_pair(db.desc[0], np.zeros((0, 32), np.uint8), 255) == 0 and P.score_pair(np.zeros((0, 32), np.uint8), db.desc[0], 255) == 0


def test_gap_boundary_and_sequences():
    db = _db()
    # frames 0, 5, 9: frame_c <= frame_q - min_gap
    assert (db.score(2, 1, 4, min_gap=4)[0] >= 0).tolist() == [True, True, False]     # 5 <= 9 - 4
    assert (db.score(2, 1, 4, min_gap=5)[0] >= 0).tolist() == [True, False, False]    # 5 >  9 - 5
    assert (db.score(2, 1, 4, min_gap=9)[0] >= 0).tolist() == [True, False, False]    # 0 <= 9 - 9
    assert (db.score(2, 1, 4, min_gap=10)[0] >= 0).tolist() == [False, False, False]
    assert (db.score(2, 1, 4, min_gap=0)[0] >= 0).tolist() == [True, True, True]      # min_gap 0: itself too
    db.seq[0] = 7                                                                     # another sequence is never eligible
    assert (db.score(2, 1, 4, min_gap=1)[0] >= 0).tolist() == [False, True, False]


def test_select_ties_min_score_and_k_above_eligible():
    score = np.array([[5, -1, 7, 5, 0, 7, 3],
                      [-1, -1, -1, -1, -1, -1, -1],
                      [0, 0, -1, 0, -1, -1, -1]], np.int32)
    cand, cs = P.select(score, K=3, min_score=1)
    assert cand[0].tolist() == [2, 5, 0] and cs[0].tolist() == [7, 7, 5]              # ties to the smaller id
    assert cand[1].tolist() == [-1, -1, -1] and cs[1].tolist() == [0, 0, 0]
    assert cand[2].tolist() == [-1, -1, -1]                                           # score 0 does not reach min_score 1
    cand, cs = P.select(score, K=8, min_score=0)                                      # K above the number of eligible entries
    assert cand[0].tolist() == [2, 5, 0, 3, 6, 4, -1, -1] and cs[0].tolist() == [7, 7, 5, 5, 3, 0, 0, 0]
    assert cand[2].tolist() == [0, 1, 3, -1, -1, -1, -1, -1]
    cand, _ = P.select(score, K=2, min_score=-5)                                      # a pair that is not eligible is never a candidate
    assert cand[1].tolist() == [-1, -1]
    cand, cs = P.select(score, K=4, min_score=5)                                      # the boundary: 5 reaches 5
    assert cand[0].tolist() == [2, 5, 0, 3]
    assert P.select(score, K=4, min_score=6)[0][0].tolist() == [2, 5, -1, -1]


def test_add_mask_clamp_and_refusal():
    rng = np.random.default_rng(3)
    descs = [rng.integers(0, 256, (6, 32), dtype=np.uint8) for _ in range(4)]
    valids = [np.array([1, 0, 1, 1, 0, 1], np.uint8)] * 4
    db = P.PlaceRef(rows=4, capacity=3)
    assert db.add(descs, [6, 2, 0, 5], [0, 0, 1, 1], [10, 11, 12, 13], add=[1, 0, 1, 1], valids=valids) == 0
    assert len(db) == 3 and [len(d) for d in db.desc] == [4, 0, 4] and db.frame == [10, 12, 13] and db.seq == [0, 1, 1]
    assert np.array_equal(db.desc[0], descs[0][:4]) and np.array_equal(db.desc[2], descs[3][:4])
    assert db.qsel(0).tolist() == [0, 2, 3] and db.qsel(1).tolist() == []
    before = [d.copy() for d in db.desc]
    assert db.add(descs[:1], [3], [0], [14]) is None and db.n_refused == 1 and len(db) == 3
    assert all(np.array_equal(a, b) for a, b in zip(before, db.desc))
    assert db.add(descs, [1, 1, 1, 1], [0] * 4, [0] * 4, add=[0, 0, 0, 0]) == 3 and len(db) == 3 and db.n_refused == 1
