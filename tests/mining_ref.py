"""Hard / semi-hard negative mining restated on the host (test infrastructure; never imported by the product path).

The semantics of include/tsgnn.h's mining section, written from that description: the class of an entry's drawn negative is the
negative class, its candidates are ``members[class_ptr[c] : class_ptr[c + 1]]`` in that order.
  mode 2 (hardest)    start from the drawn negative, walk the candidates in list order, take one only when strictly closer than the
                      best so far
  mode 1 (semi-hard)  the first candidate in list order closer to the anchor than the positive is; none: the drawn negative stays

``mine_loop``   one ``np.linalg.norm`` call per (anchor, candidate) pair on float64 rows: the shape of the reference's own loop (and the
                host baseline scripts/mining_epoch.py times)
``mine``        the same walk on squared float64 distances, one numpy expression per entry (also the vectorised host baseline)
``mine_int``    for integer-valued embeddings: int64 arithmetic, exact whatever the order of summation
All three return a NEW [T, 3] int64 schedule; ``changed`` counts the entries whose negative differs."""
import numpy as np

SEMI_HARD, HARDEST = 1, 2


def _tables(class_of, class_ptr, members):
    return np.asarray(class_of, dtype=np.int64), np.asarray(class_ptr, dtype=np.int64), np.asarray(members, dtype=np.int64)


def mine_loop(emb, sched, class_of, class_ptr, members, mode):
    X = np.asarray(emb, dtype=np.float64)
    class_of, class_ptr, members = _tables(class_of, class_ptr, members)
    out = np.array(sched, dtype=np.int64)
    for row in out:
        a, p, n = (int(v) for v in row)
        c = class_of[n]
        cand = members[class_ptr[c]:class_ptr[c + 1]]
        if mode == SEMI_HARD:
            bound = np.linalg.norm(X[a] - X[p])
            for j in cand:
                if np.linalg.norm(X[a] - X[j]) < bound:
                    row[2] = j
                    break
        else:
            best = np.linalg.norm(X[a] - X[n])
            for j in cand:
                d = np.linalg.norm(X[a] - X[j])
                if d < best:
                    best, row[2] = d, j
    return out


def d2(X, a, rows):
    """squared distances of row ``a`` to ``rows`` in X's own arithmetic (float64 or int64)"""
    diff = X[rows] - X[a]
    return (diff * diff).sum(-1)


def _walk(X, sched, class_of, class_ptr, members, mode):
    class_of, class_ptr, members = _tables(class_of, class_ptr, members)
    out = np.array(sched, dtype=np.int64)
    for row in out:
        a, p, n = (int(v) for v in row)
        c = class_of[n]
        cand = members[class_ptr[c]:class_ptr[c + 1]]
        if cand.size == 0:
            continue
        d = d2(X, a, cand)
        if mode == SEMI_HARD:
            hit = np.flatnonzero(d < d2(X, a, p))
            if hit.size:
                row[2] = cand[hit[0]]
        else:
            # strictly below the drawn negative, then the first position of the minimum (np.argmin: the first occurrence)
            if d.min() < d2(X, a, n):
                row[2] = cand[int(np.argmin(d))]
    return out


def mine(emb, sched, class_of, class_ptr, members, mode):
    return _walk(np.asarray(emb, dtype=np.float64), sched, class_of, class_ptr, members, mode)


def mine_f32(emb, sched, class_of, class_ptr, members, mode):
    """the same walk in float32 numpy (difference form, numpy's own summation order): what fp32 rounding alone does to the choice"""
    return _walk(np.asarray(emb, dtype=np.float32), sched, class_of, class_ptr, members, mode)


def mine_int(emb, sched, class_of, class_ptr, members, mode):
    E = np.asarray(emb)
    X = np.rint(E).astype(np.int64)
    if not np.array_equal(X, E):
        raise ValueError("mine_int takes integer-valued embeddings")
    return _walk(X, sched, class_of, class_ptr, members, mode)


def changed(before, after):
    return int((np.asarray(before)[:, 2] != np.asarray(after)[:, 2]).sum())


def tie_counts(emb, sched, class_of, class_ptr, members):
    """(hardest, semi-hard): entries whose outcome rests on the tie rules — hardest: the minimum over {drawn negative} + candidates
    is attained at two or more places that are different graphs' list positions (or the drawn negative and another position);
    semi-hard: a candidate at or before the chosen position (any position when none is chosen) lies at EXACTLY the positive's distance,
    so '<' against '<=' decides"""
    X = np.asarray(emb, dtype=np.float64)
    class_of, class_ptr, members = _tables(class_of, class_ptr, members)
    hard = semi = 0
    for a, p, n in np.asarray(sched, dtype=np.int64):
        cand = members[class_ptr[class_of[n]]:class_ptr[class_of[n] + 1]]
        if cand.size == 0:
            continue
        d = d2(X, a, cand)
        dn, dp = d2(X, a, n), d2(X, a, p)
        m = min(d.min(), dn)
        at = np.flatnonzero(d == m)
        places = at.size + (1 if dn == m and not (cand[at] == n).any() else 0)
        hard += int(places >= 2)
        hit = np.flatnonzero(d < dp)
        upto = hit[0] if hit.size else cand.size
        semi += int((d[:upto + 1] == dp).any())
    return hard, semi


def tau(E):
    """relative band of a comparison of two fp32 difference-form sums of E non-negative terms: each is off by at most
    (E + 2) 2^-24 relative (E roundings of the running sum, the subtraction and the square of a term)"""
    return 2.0 * (E + 2) * 2.0 ** -24


def acceptable(emb, entry, choice, class_of, class_ptr, members, mode, t):
    """is ``choice`` an answer for schedule ``entry`` (a, p, drawn n) that fp32 arithmetic within the band ``t`` may give?  (float64
    distances of the given rows)"""
    X = np.asarray(emb, dtype=np.float64)
    class_of, class_ptr, members = _tables(class_of, class_ptr, members)
    a, p, n = (int(v) for v in entry)
    cand = members[class_ptr[class_of[n]]:class_ptr[class_of[n] + 1]]
    d = d2(X, a, cand)
    if mode == HARDEST:
        if choice != n and choice not in cand:
            return False
        return bool(d2(X, a, choice) <= (1 + t) * min(d.min(), d2(X, a, n)))
    dp = d2(X, a, p)
    if choice == n and bool((d >= (1 - t) * dp).all()):
        return True                                                              # kept: no position clearly qualifies
    at = np.flatnonzero(cand == choice)
    if at.size == 0:
        return False
    pos = int(at[0])
    return bool(d[pos] < (1 + t) * dp and (d[:pos] >= (1 - t) * dp).all())
