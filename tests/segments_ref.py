"""Helpers of the segment tests (vslam_set_segments: several independent sequences in one batch).  The yardstick for a segment is the existing
path on that segment alone, so the helpers only cut concatenated tables into per-segment tables and paste per-segment results back together."""
import numpy as np

# window arrays indexed by landmark / by edge / by window, and the ones that hold batch frame indices (-1: none)
PER_LM = ("xyz", "reliable", "lm_inlier")
PER_EDGE = ("kf_idx", "lm_idx", "uv")
PER_WINDOW = ("n_kf", "T", "kf_frame", "evicted", "state", "pred", "nmem")
FRAME_INDEX = ("kf_frame", "evicted", "pred")


def split_tables(tables, first):
    """tables: {name: array}; the arrays of the longest leading dimension F are per frame, those of F - 1 per frame pair (item i = the pair
    i -> i + 1).  Returns one dict per segment: per-frame rows [first[k], first[k + 1]), per-pair rows [first[k], first[k + 1] - 1) -- the pair
    before a segment's first frame belongs to no segment."""
    first = [int(x) for x in first]
    F = first[-1]
    out = []
    for lo, hi in zip(first[:-1], first[1:]):
        seg = {}
        for k, a in tables.items():
            if len(a) == F:
                seg[k] = a[lo:hi]
            elif len(a) == F - 1:
                seg[k] = a[lo:hi - 1]
            else:
                raise ValueError("%s: leading dimension %d is neither %d frames nor %d pairs" % (k, len(a), F, F - 1))
        out.append(seg)
    return out


def concat_windows(parts):
    """parts: per-segment window dicts (lm_off / edge_off of n + 1 entries, the per-landmark and per-edge arrays, per-window arrays, status).
    Returns the dict of the batch that holds the segments back to back: offsets rebased onto the concatenated arrays, the per-landmark and
    per-edge arrays cut to each part's totals and joined, frame indices shifted by the segment's first frame, status ORed."""
    out = {}
    lm_off, e_off = [np.zeros(1, np.int32)], [np.zeros(1, np.int32)]
    nl = ne = f0 = 0
    for p in parts:
        n = len(p["lm_off"]) - 1
        lm_off.append(p["lm_off"][1:] + nl); e_off.append(p["edge_off"][1:] + ne)
        pl, pe = int(p["lm_off"][n]), int(p["edge_off"][n])
        for k in PER_LM:
            if k in p:
                out.setdefault(k, []).append(p[k][:pl])
        for k in PER_EDGE:
            if k in p:
                out.setdefault(k, []).append(p[k][:pe])
        for k in PER_WINDOW:
            if k in p:
                a = np.asarray(p[k])
                out.setdefault(k, []).append(np.where(a >= 0, a + f0, a) if k in FRAME_INDEX else a)
        nl += pl; ne += pe; f0 += n
    out = {k: np.concatenate(v) for k, v in out.items()}
    out["lm_off"] = np.concatenate(lm_off).astype(np.int32); out["edge_off"] = np.concatenate(e_off).astype(np.int32)
    out["status"] = int(np.bitwise_or.reduce([int(p.get("status", 0)) for p in parts]))
    return out
