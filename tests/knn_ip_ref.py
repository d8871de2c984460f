"""TEST INFRASTRUCTURE -- the oracle of the inner-product search (ac_knn_ip_topk, faiss.IndexFlatIP.search).

    v(q, n) = sum_c float64(P[n,c]) * float64(Q[q,c])      every product of two fp32 values is exact in fp64; the sum runs over
                                                           c = 0, 1, ..., D-1 in that fixed order for every row, so identical
                                                           rows get identical values (exact ties stay exact ties)
    order by (v descending, n ascending); returned value = float32(v); k > N pads with (-FLT_MAX, -1), -inf in fp64

Large shapes may shortlist with a BLAS fp64 product (`knn_ip_topk_shortlisted`): the shortlist is re-evaluated with the
fixed-order sum, and the function returns, per query, how far the shortlist's cut-off lies below the k-th exact value together
with the bound 1e-9 |p|max |q| the caller must assert it exceeds (a BLAS fp64 dot of D <= 4096 terms is off by less than
D 2^-53 |p||q| < 1e-12 |p||q|, so a row outside such a shortlist cannot belong to the top-k).
"""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def fixed_order_ip(P64, Q64):
    """[nq, n] fp64 inner products, summed over the columns in index order.  P64 [n, D] or [nq, n, D] (per-query rows)."""
    per_query = P64.ndim == 3
    nq, n = Q64.shape[0], P64.shape[-2]
    acc = np.zeros((nq, n), dtype=np.float64)
    for c in range(Q64.shape[1]):
        acc += (P64[:, :, c] if per_query else P64[None, :, c]) * Q64[:, c:c + 1]
    return acc


def _select(vals, ids, k, row_offset, outD, outE, outI, q):
    """(value descending, id ascending) top-k of one query's candidates into row q of the outputs"""
    kk = min(k, vals.shape[0])
    if kk == 0:
        return
    if kk < vals.shape[0]:
        kth = np.partition(vals, vals.shape[0] - kk)[vals.shape[0] - kk]
        keep = vals >= kth
        vals, ids = vals[keep], ids[keep]
    order = np.lexsort((ids, -vals))[:kk]
    outD[q, :kk] = vals[order].astype(np.float32)
    outE[q, :kk] = vals[order]
    outI[q, :kk] = ids[order] + row_offset


def _outputs(nq, k):
    return (np.full((nq, k), -FLT_MAX, dtype=np.float32), np.full((nq, k), -np.inf, dtype=np.float64),
            np.full((nq, k), -1, dtype=np.int64))


def knn_ip_topk(P, Q, k, row_offset=0, return_exact=False):
    """(float32 [nq,k], int64 [nq,k]); return_exact=True: (float64 exact values padded with -inf, ids) -- what one row shard
    contributes to a sharded search.  Every row is evaluated with the fixed-order sum."""
    P = np.asarray(P, dtype=np.float32)
    Q = np.asarray(Q, dtype=np.float32)
    nq, N = Q.shape[0], P.shape[0]
    outD, outE, outI = _outputs(nq, k)
    if N and nq:
        ids = np.arange(N, dtype=np.int64)
        Q64 = Q.astype(np.float64)
        for s in range(0, nq, 64):
            v = fixed_order_ip(P.astype(np.float64), Q64[s:s + 64])
            for q in range(v.shape[0]):
                _select(v[q], ids, k, row_offset, outD, outE, outI, s + q)
    return (outE, outI) if return_exact else (outD, outI)


def knn_ip_topk_shortlisted(P, Q, k, row_offset=0, extra=64):
    """For large shapes: (float32 [nq,k], ids [nq,k], gap [nq], bound [nq]).  A BLAS fp64 product shortlists the k + extra
    best rows per query; those are re-evaluated with the fixed-order sum and ordered as in knn_ip_topk.  gap[q] = (k-th exact
    value) - (largest BLAS value outside the shortlist), bound[q] = 1e-9 |p|max |q|: the CALLER asserts gap > bound."""
    P = np.asarray(P, dtype=np.float32)
    Q = np.asarray(Q, dtype=np.float32)
    nq, N = Q.shape[0], P.shape[0]
    m = k + extra
    assert N > m, "shortlisting needs more rows than the shortlist holds"
    Q64 = Q.astype(np.float64)
    S = np.empty((nq, N), dtype=np.float64)
    pmax2 = 0.0
    for s in range(0, N, 65536):
        P64 = P[s:s + 65536].astype(np.float64)
        S[:, s:s + 65536] = Q64 @ P64.T
        pmax2 = max(pmax2, float(np.einsum("nc,nc->n", P64, P64).max()))
    part = np.argpartition(-S, m, axis=1)                        # columns [0, m) = the m largest, column m = the next one
    short = np.sort(part[:, :m], axis=1).astype(np.int64)
    cutoff = S[np.arange(nq), part[:, m]]
    outD, outE, outI = _outputs(nq, k)
    for s in range(0, nq, 64):
        rows = P[short[s:s + 64]].astype(np.float64)             # [b, m, D]
        v = fixed_order_ip(rows, Q64[s:s + 64])
        for q in range(v.shape[0]):
            _select(v[q], short[s + q], k, row_offset, outD, outE, outI, s + q)
    gap = outE[:, k - 1] - cutoff
    bound = 1e-9 * np.sqrt(pmax2) * np.sqrt(np.einsum("qc,qc->q", Q64, Q64))
    return outD, outI, gap, bound


def topk_merge_ip(D_in, I_in, k):
    """Oracle for ac_topk_merge_ip_f64: [shards, nq, k] descending fp64 lists -> global top-k by (value descending, id
    ascending), values rounded to float32; entries with id < 0 are padding."""
    D_in = np.asarray(D_in, dtype=np.float64)
    I_in = np.asarray(I_in, dtype=np.int64)
    nq = D_in.shape[1]
    outD = np.full((nq, k), -FLT_MAX, dtype=np.float32)
    outI = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        d, i = D_in[:, q, :].reshape(-1), I_in[:, q, :].reshape(-1)
        d, i = d[i >= 0], i[i >= 0]
        order = np.lexsort((i, -d))[:k]
        outD[q, :len(order)] = d[order]
        outI[q, :len(order)] = i[order]
    return outD, outI
