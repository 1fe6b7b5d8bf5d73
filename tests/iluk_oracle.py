"""CPU restatement of the level-of-fill ILU(k) pattern as include/psk.h defines it for psk_csr_iluk_pattern (TEST
INFRASTRUCTURE).

The sequential definition, statement by statement (the device builds the same pattern in k row-parallel rounds):

    work on the copy S of A whose rows are in ascending column order; every stored entry has level 0
    for i = 0 .. n-1:
      for each entry (i, c) of row i with c < i, in ascending c, fill entries included as this pass adds them:
        for every entry (c, j) of the finished row c with j > c:
          cand = lev(i,c) + lev(c,j) + 1
          if cand <= k and (i, j) is absent or holds a larger level: lev(i,j) = cand

P = the entries with lev <= k, rows ascending, A's value where A stores the entry and +0.0 at a fill entry; Lev the
same structure with the levels as doubles. The ILU(k) factor is ilu0_oracle.ilu0(P).
"""
import heapq

import numpy as np
import scipy.sparse as sp

import ilu0_oracle as io0

MAX_LEVEL = 8


def pattern(A, k):
    """(P, Lev) as scipy CSR with sorted rows. ValueError for a matrix that is not square, a duplicate column, a
    missing diagonal or a k outside [0, MAX_LEVEL]."""
    if isinstance(k, bool) or int(k) != k or not 0 <= k <= MAX_LEVEL:
        raise ValueError("k must be an integer in [0, %d]" % MAX_LEVEL)
    S = io0.sorted_copy(A)
    n, nc = S.shape
    if n != nc or n == 0:
        raise ValueError("ILU(k) needs a square, non-empty matrix")
    rp, ci, va = S.indptr.tolist(), S.indices.tolist(), S.data.tolist()
    rows = []      # finished rows: (columns ascending, levels, position of the first column > row)
    out_c, out_l, out_v, out_p = [], [], [], [0]
    for i in range(n):
        cols = ci[rp[i]:rp[i + 1]]
        if len(set(cols)) != len(cols):
            raise ValueError("duplicate column in row %d" % i)
        if i not in cols:
            raise ValueError("row %d has no stored diagonal entry" % i)
        lev = {c: 0 for c in cols}
        val = dict(zip(cols, va[rp[i]:rp[i + 1]]))
        todo = [c for c in cols if c < i]          # the lower entries still to visit, a heap: ascending c
        heapq.heapify(todo)
        while todo:
            c = heapq.heappop(todo)
            ccols, clev, up = rows[c]
            lic = lev[c]
            for q in range(up, len(ccols)):
                j = ccols[q]
                cand = lic + clev[q] + 1
                if cand <= k and (j not in lev or lev[j] > cand):
                    if j not in lev and j < i:     # j > c: a lower entry this pass has not reached yet
                        heapq.heappush(todo, j)
                    lev[j] = cand
        srt = sorted(lev)
        lv = [lev[c] for c in srt]
        rows.append((srt, lv, next(q for q, c in enumerate(srt) if c == i) + 1))
        out_c.extend(srt)
        out_l.extend(float(x) for x in lv)
        out_v.extend(val.get(c, 0.0) for c in srt)
        out_p.append(len(out_c))
    ip, ix = np.array(out_p, dtype=np.int32), np.array(out_c, dtype=np.int32)
    P = sp.csr_matrix((np.array(out_v, dtype=np.float64), ix, ip), shape=(n, n))
    Lev = sp.csr_matrix((np.array(out_l, dtype=np.float64), ix.copy(), ip.copy()), shape=(n, n))
    P.has_sorted_indices = Lev.has_sorted_indices = True
    return P, Lev


def iluk(A, k):
    """The ILU(k) factor F (scipy CSR, sorted rows): ILU(0) of the padded matrix, in ilu0_oracle's arithmetic."""
    return io0.ilu0(pattern(A, k)[0])
