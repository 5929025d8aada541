"""Exact numpy restatement of the place database's rules (include/vslam_hip.h "place database"): the score, eligibility, candidate selection and
the add bookkeeping.  Everything is integer arithmetic, so the device results must equal these bit for bit."""
import numpy as np


def hamming_table(a, b):
    """(len(a), len(b)) int32 Hamming distances of 32-byte descriptor rows: unpacked bits, one integer matrix product"""
    A = np.unpackbits(np.ascontiguousarray(a, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    B = np.unpackbits(np.ascontiguousarray(b, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    # hamming = |a| + |b| - 2 <a, b>
    return A.sum(1)[:, None] + B.sum(1)[None, :] - 2 * (A @ B.T)


def score_pair(Di, Dj, tau):
    """#{ r : min_c hamming(Di[r], Dj[c]) <= tau }; 0 when either side is empty"""
    if len(Di) == 0 or len(Dj) == 0:
        return 0
    return int((hamming_table(Di, Dj).min(axis=1) <= tau).sum())


def eligible(seq_q, frame_q, seq_c, frame_c, min_gap):
    return seq_c == seq_q and frame_c <= frame_q - min_gap


class PlaceRef:
    """the database: entries are (descriptor rows clamped to R, seq, frame[, valid flags clamped to R])"""

    def __init__(self, rows, capacity):
        self.rows, self.capacity = int(rows), int(capacity)
        self.desc, self.seq, self.frame, self.valid = [], [], [], []
        self.n_refused = 0

    def __len__(self):
        return len(self.desc)

    def add(self, descs, ns, seqs, frames, add=None, valids=None):
        """items b with add[b] != 0 (None: all), ascending b, the first min(ns[b], R) rows each; an add that does not fit adds nothing and is counted.
        Returns the id of the first entry added, or None when refused."""
        B = len(descs)
        take = [b for b in range(B) if add is None or add[b] != 0]
        first = len(self)
        if first + len(take) > self.capacity:
            self.n_refused += 1
            return None
        for b in take:
            n = min(max(int(ns[b]), 0), self.rows)
            self.desc.append(np.ascontiguousarray(descs[b][:n], np.uint8).reshape(-1, 32).copy())
            self.seq.append(int(seqs[b])); self.frame.append(int(frames[b]))
            self.valid.append(None if valids is None else np.asarray(valids[b][:n], np.uint8).copy())
        return first

    def qsel(self, e):
        """the ascending rows of entry e that own a valid point"""
        return np.flatnonzero(self.valid[e]).astype(np.int32)

    def score(self, q0, nq, tau, min_gap):
        """(nq, n_entries) int32: -1 where the pair is not eligible"""
        out = np.full((nq, len(self)), -1, np.int32)
        for i in range(nq):
            e = q0 + i
            for j in range(len(self)):
                if eligible(self.seq[e], self.frame[e], self.seq[j], self.frame[j], min_gap):
                    out[i, j] = score_pair(self.desc[e], self.desc[j], tau)
        return out


def select(score, K, min_score):
    """per row of a score table the K eligible (score >= 0) entries with the highest score that reach min_score: descending score, ties to the smaller
    entry id; unused slots -1 / 0.  Returns (cand, cand_score), each (nq, K) int32."""
    score = np.asarray(score, np.int32)
    cand = np.full((len(score), K), -1, np.int32); cs = np.zeros((len(score), K), np.int32)
    for i, row in enumerate(score):
        ok = np.flatnonzero((row >= 0) & (row >= min_score))
        order = ok[np.lexsort((ok, -row[ok].astype(np.int64)))][:K]
        cand[i, :len(order)] = order; cs[i, :len(order)] = row[order]
    return cand, cs
