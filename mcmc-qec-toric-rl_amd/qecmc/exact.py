"""The exact class law by coset enumeration on the device (qecmc_coset_enumerate; no counterpart in the reference, whose decoders all estimate
this quantity): for every syndrome the integer histogram hist[c, n_xy, n_z] of the chains of class c over their X-or-Y and Z counts, summed over
the whole stabilizer group, and from it the class weights Z_c = sum hist[c] * w(n_xy, n_z) of any noise model whose weight is a function of the two
counts -- the maximum-likelihood decoder of the small codes (toric L = 3, planar L = 3, 4, xzzx / rotated L = 3, 5).

The same law by a frontier sweep (qecmc_class_sweep): the class weights themselves, float64, for four per-qubit weights of I, X, Y
and Z, by variable elimination across the lattice -- which reaches xzzx / rotated L = 9 and planar L = 6.

The sweep past one LDS state vector (qecmc_class_sweep_cut): generators held out of the elimination and summed over by workgroups --
which reaches the toric code at L = 5, and with a 128 KiB state vector xzzx / rotated L = 11 and planar L = 7.

The sweep on a state vector tiled over HBM (qecmc_class_sweep_tiled): the state vector of a (syndrome, class) lives in a device
workspace and passes through LDS one tile per workgroup, one launch per segment of the op stream -- which reaches xzzx / rotated L = 21, planar
L = 12 and, with five generators held, the toric code at L = 7.  It runs only where it is named (method="tiled"): "auto" routes as before.

The three sweeps under a weight per (syndrome, qubit) (qecmc_class_sweep_site, _cut_site, _tiled_site): class_sweep_site and
exact_site_probabilities take a table of weights in place of the four numbers -- erasures (erasure_site_w4), a map of error rates
(depolarizing_site_w4, biased_site_w4), any per-shot prior -- at every shape the uniform sweeps reach.

The shortest chain of every class and its multiplicity (qecmc_class_minplus): the cut-set sweep's plans in the semiring of
(cost, count) pairs under (min, +), integer and exact -- class_minplus, the minimum-weight decoder min_weight_classes, and shortest_class_law, the
exact value of what the shortest-chain estimators converge to.

That sweep traced back to a chain (qecmc_class_minplus_chains): shortest_chains returns a shortest chain of every class next to
cost and count, min_weight_corrections the minimum-weight decoder's correction.

Both under a cost per (syndrome, qubit) (qecmc_class_minplus_site, qecmc_class_minplus_chains_site): class_minplus_site,
shortest_chains_site, min_weight_classes_site and min_weight_corrections_site take a table of integer costs in place of the four numbers --
erasures (erasure_site_costs), integer log-likelihoods of any site weights (llr_site_costs): the most likely chain of a class, exactly.

Exact draws (qecmc_class_sample, qecmc_class_sample_site): the cut-set sweep run forward with a record of every FORGET and walked back
with one uniform per generator -- sample_chains and sample_chains_site draw independent chains of every class with probability w(chain) / Z_c,
sample_posterior draws the class first, posterior_error_counts is the exact yardstick of a sampler's mean error count.

Exact marginals (qecmc_class_marginals, qecmc_class_marginals_site): the same forward sweep with a record of every CLOSE and a
backward sweep over the same stream -- class_marginals and class_marginals_site give, per class, the weight with which every qubit carries I, X, Y
or Z; posterior_marginals mixes the classes with Z_c / Z; exact_error_counts is the exact value of what posterior_error_counts estimates.

Exact draws on the tiled route (qecmc_class_sample_tiled, _tiled_site): sample_chains_tiled and sample_chains_tiled_site draw at the
shapes past the cut plans (xzzx / rotated L = 13 .. 17 under the default record cap); sample_posterior and posterior_error_counts take
method="tiled".

The traceback on the tiled route (qecmc_class_minplus_tiled_chains, _chains_site): shortest_chains_tiled and
shortest_chains_tiled_site return a shortest chain of every class at the shapes only the tiled sweep takes; min_weight_corrections and
min_weight_corrections_site reach them with method="tiled"."""
import ctypes as C

import numpy as np

from . import _lib as L_

_CODES = {"toric": L_.TORIC, "xzzx": L_.XZZX, "rotated": L_.ROTATED, "planar": L_.PLANAR}


def enumerator_info(code, size):
    """dict(rank, ncls, nq, chunk_bits: the default) of one (code, size), from the host half of the library alone; raises QecmcError where the
    enumeration refuses the code"""
    v = [C.c_int32() for _ in range(4)]
    L_.check(L_.lib().qecmc_coset_enumerate_info(_CODES.get(code, code), int(size), *[C.byref(x) for x in v]))
    return dict(zip(("rank", "ncls", "nq", "chunk_bits"), (int(x.value) for x in v)))


def _as_chains(code, chains, size):
    """chains -> (uint8[N, nq], L).  [N, ...] or one [...] with ... the code's qubit_matrix shape; with `size` given also the flat [N, nq]."""
    a = np.ascontiguousarray(chains, dtype=np.uint8)
    sd = 3 if code in (L_.TORIC, L_.PLANAR) else 2
    if size is not None and a.ndim == 2 and a.shape[-1] == (2 if sd == 3 else 1) * size * size:
        return a, int(size)
    if a.ndim == sd:
        a = a[None]
    if a.ndim != sd + 1 or a.shape[-1] != a.shape[-2] or (sd == 3 and a.shape[-3] != 2) or (size is not None and size != a.shape[-1]):
        raise ValueError(f"chains of shape {a.shape} are not [N, ...] configurations of this code" + ("" if size is None else f" at size {size}"))
    return a.reshape(a.shape[0], -1), a.shape[-1]


def coset_enumerator(code, chains, size=None, chunk_bits=0, chunks=None, device=0):
    """The histogram of every syndrome, on the GPU.  code: "toric" / "xzzx" / "rotated" / "planar" (or the qecmc code number); chains uint8[N, ...]:
    one chain per syndrome (any chain with it: hist depends on the syndrome alone).  chunk_bits (0: the
    default) cuts the 2^rank group elements into chunks of 2^chunk_bits; chunks=(first, count) enumerates that range only -- partial histograms over
    disjoint ranges add up to the whole.
    Returns dict(hist uint64[N, ncls, nq+1, nq+1], cls int32[N]: the class of each input chain, rank)."""
    code = _CODES.get(code, code)
    if int(device) != 0:
        raise ValueError("coset_enumerator runs on device 0: the library has no device-pointer form of it yet")
    flat, L = _as_chains(code, chains, size)
    info = enumerator_info(code, L)
    n, nq1 = flat.shape[0], info["nq"] + 1
    first, count = (0, 0) if chunks is None else (int(chunks[0]), int(chunks[1]))
    if chunks is not None and count < 1:
        raise ValueError(f"chunks={chunks!r}: (first, count) with count >= 1")
    hist = np.zeros((n, info["ncls"], nq1, nq1), dtype=np.uint64)
    cls = np.zeros(n, dtype=np.int32)
    L_.check(L_.lib().qecmc_coset_enumerate(code, L, n, L_.u8(flat), int(chunk_bits), first, count, hist.ctypes.data_as(L_._u64p), L_.i32(cls)))
    return dict(hist=hist, cls=cls, rank=info["rank"])


def sweep_info(code, size):
    """dict(width, ncls, nq, n_ops) of the sweep plan of one (code, size), from the host half of the library alone; raises QecmcError where the
    sweep refuses the code"""
    v = [C.c_int32() for _ in range(4)]
    L_.check(L_.lib().qecmc_class_sweep_info(_CODES.get(code, code), int(size), *[C.byref(x) for x in v]))
    return dict(zip(("width", "ncls", "nq", "n_ops"), (int(x.value) for x in v)))


def class_sweep(code, chains, weights, size=None, device=0):
    """The class weights of every syndrome, on the GPU.  code and chains as coset_enumerator takes them; weights: the four weights of I, X, Y and Z
    at one qubit, finite and > 0 (depolarizing_w4 / biased_w4 / alpha_w4, or any other).
    Returns dict(Z float64[N, ncls]: Z[s, c] = the sum over the chains of class c with the syndrome of chain s of the product of the weights of their
    Paulis, cls int32[N]: the class of each input chain, width: the widest frontier of the plan).  Z is raw: what IEEE double arithmetic gives with no
    rescaling, so it may be subnormal, 0 or inf; law_from_class_weights (exact_class_probabilities) is where that is judged."""
    code = _CODES.get(code, code)
    if int(device) != 0:
        raise ValueError("class_sweep runs on device 0: the library has no device-pointer form of it yet")
    flat, L = _as_chains(code, chains, size)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (4,):
        raise ValueError(f"weights of shape {w.shape}: the four weights of I, X, Y and Z")
    info = sweep_info(code, L)
    n = flat.shape[0]
    z = np.zeros((n, info["ncls"]), dtype=np.float64)
    cls = np.zeros(n, dtype=np.int32)
    f64p = C.POINTER(C.c_double)
    L_.check(L_.lib().qecmc_class_sweep(code, L, n, L_.u8(flat), w.ctypes.data_as(f64p), z.ctypes.data_as(f64p), L_.i32(cls)))
    return dict(Z=z, cls=cls, width=info["width"])


def sweep_cut_info(code, size, lds_width=0):
    """dict(full_width, width, held, ncls, nq, n_ops) of the cut-set plan of one (code, size) for a state vector of at most 2^lds_width doubles in LDS
    (0: the library's default), from the host half of the library alone; raises QecmcError where the plan is refused"""
    v = [C.c_int32() for _ in range(6)]
    L_.check(L_.lib().qecmc_class_sweep_cut_info(_CODES.get(code, code), int(size), int(lds_width), *[C.byref(x) for x in v]))
    return dict(zip(("full_width", "width", "held", "ncls", "nq", "n_ops"), (int(x.value) for x in v)))


def class_sweep_cut(code, chains, weights, size=None, lds_width=0):
    """class_sweep past one LDS state vector (qecmc_class_sweep_cut): `held` generators are held out of the elimination and summed over
    by 2^held workgroups per (class, syndrome) -- the toric code at L = 5, and with nothing held xzzx / rotated L = 11 and planar L = 7 at width 14.
    lds_width: the widest state vector a workgroup may hold, 2 .. 14, 0: the default.
    Returns dict(Z float64[N, ncls], cls int32[N], width: the widest frontier of the cut plan, held: the number of held generators).  Z is raw, as
    class_sweep's: it may be subnormal, 0 or inf, and law_from_class_weights is where that is judged."""
    code = _CODES.get(code, code)
    flat, L = _as_chains(code, chains, size)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (4,):
        raise ValueError(f"weights of shape {w.shape}: the four weights of I, X, Y and Z")
    info = sweep_cut_info(code, L, lds_width)
    n = flat.shape[0]
    z = np.zeros((n, info["ncls"]), dtype=np.float64)
    cls = np.zeros(n, dtype=np.int32)
    f64p = C.POINTER(C.c_double)
    L_.check(L_.lib().qecmc_class_sweep_cut(code, L, n, L_.u8(flat), w.ctypes.data_as(f64p), int(lds_width), z.ctypes.data_as(f64p), L_.i32(cls)))
    return dict(Z=z, cls=cls, width=info["width"], held=info["held"])


def class_minplus(code, chains, costs=(0, 1, 1, 1), size=None, lds_width=0):
    """The least cost of every class of every syndrome and the number of chains that reach it, on the GPU (qecmc_class_minplus):
    class_sweep_cut's plans run in the semiring of (cost, count) pairs under (min, +), in integers.  code and chains as class_sweep_cut takes them;
    costs: the integer costs of I, X, Y and Z at one qubit, 0 .. 255 each (the default counts the errors of a chain); lds_width as
    class_sweep_cut's.  Shapes: toric L = 3, 5, planar L = 3 .. 7, xzzx / rotated L = 3 .. 11.
    Returns dict(cost uint32[N, ncls]: the least sum of costs over the chains of class c with the syndrome of chain s, count uint64[N, ncls]: how many
    chains of the class reach it -- 0 where saturated --, saturated bool[N, ncls]: the count passed 2^48 - 1 on the way (on the torus 2^46 - 1: the
    generator table meets every chain four times) and is not known, cls int32[N]: the class of each input chain, width, held: the cut plan's)."""
    code = _CODES.get(code, code)
    flat, L = _as_chains(code, chains, size)
    c = np.asarray(costs, dtype=np.float64)
    if c.shape != (4,) or not np.all((c >= 0) & (c <= 0xFFFFFFFF) & (c == np.floor(c))):
        raise ValueError(f"costs={costs!r}: the four integer costs of I, X, Y and Z, each >= 0")
    c = c.astype(np.uint32)
    n, ncls = flat.shape[0], 16 if code == L_.TORIC else 4
    cost = np.zeros((n, ncls), dtype=np.uint32)
    count = np.zeros((n, ncls), dtype=np.uint64)
    cls = np.zeros(n, dtype=np.int32)
    L_.check(L_.lib().qecmc_class_minplus(code, L, n, L_.u8(flat), c.ctypes.data_as(L_._u32p), int(lds_width), cost.ctypes.data_as(L_._u32p),
                                          count.ctypes.data_as(L_._u64p), L_.i32(cls)))
    info = sweep_cut_info(code, L, lds_width)
    return dict(cost=cost, count=count, saturated=count == 0, cls=cls, width=info["width"], held=info["held"])


def _rank_classes(cost, count):
    """int32[N]: the class of least cost, ties broken by the larger count, then by the lower class index (a saturated count, reported as 0, counts as the
    largest)"""
    cost = np.asarray(cost, dtype=np.int64)
    count = np.asarray(count, dtype=np.uint64)
    ncls = cost.shape[1]
    big = np.where(count == 0, np.uint64(1) << np.uint64(48), count)
    order = np.lexsort((np.broadcast_to(np.arange(ncls), cost.shape), -big.astype(np.int64), cost), axis=1)     # (last key first: cost, then count, then index)
    return order[:, 0].astype(np.int32)


_MINPLUS_METHODS = ("cut", "tiled")


def _minplus_by_method(code, chains, costs, site_costs, method, size=None, lds_width=0, hbm_width=0, tile_width=0):
    """class_minplus / class_minplus_site (method "cut", the default everywhere: lds_width) or class_minplus_tiled / class_minplus_tiled_site (method
    "tiled", only where it is named: hbm_width, tile_width); a width of the other route is refused by name"""
    if method not in _MINPLUS_METHODS:
        raise ValueError(f"method={method!r}: the (min, +) sweep runs on the cut plans ('cut') or tiled over HBM ('tiled')")
    if method == "cut":
        if hbm_width or tile_width:
            raise ValueError("hbm_width and tile_width belong to method='tiled'; method='cut' takes lds_width")
        return class_minplus(code, chains, costs, size=size, lds_width=lds_width) if site_costs is None else \
            class_minplus_site(code, chains, site_costs, size=size, lds_width=lds_width)
    if lds_width:
        raise ValueError("lds_width belongs to method='cut'; method='tiled' takes hbm_width and tile_width")
    return class_minplus_tiled(code, chains, costs, size=size, hbm_width=hbm_width, tile_width=tile_width) if site_costs is None else \
        class_minplus_tiled_site(code, chains, site_costs, size=size, hbm_width=hbm_width, tile_width=tile_width)


def min_weight_classes(code, chains, costs=(0, 1, 1, 1), size=None, lds_width=0, method="cut", hbm_width=0, tile_width=0):
    """int32[N]: the class class_minplus gives the least cost -- ties broken by the larger count, then by the lower class index.  At the default costs
    this is the minimum-weight decoder of depolarizing noise over Pauli chains: a Y costs 1, which matching on separate X and Z graphs cannot say.
    method="tiled" ranks class_minplus_tiled's result instead (hbm_width, tile_width as it takes them): the shapes past the cut plans."""
    r = _minplus_by_method(code, chains, costs, None, method, size=size, lds_width=lds_width, hbm_width=hbm_width, tile_width=tile_width)
    return _rank_classes(r["cost"], r["count"])


def shortest_chains(code, chains, costs=(0, 1, 1, 1), size=None, lds_width=0):
    """A shortest chain of every class of every syndrome, on the GPU (qecmc_class_minplus_chains): class_minplus's sweep traced back.
    The arguments and shapes are class_minplus's.
    Returns dict(chains uint8[N, ncls, ...]: chains[s, c] has the syndrome of chain s, lies in class c and costs cost[s, c] -- in the layout of the
    input, bytes 0 .. 3; cost, count, saturated, cls, width, held: class_minplus's, exactly; unique bool[N, ncls]: count == 1).  Where unique, the chain
    is the one shortest chain of its class and depends on the syndrome alone.  Where several chains tie, the one returned is picked by a fixed rule
    from the input chain -- a generator is applied only where that is strictly cheaper --: it is a function of (input chain, costs), and another
    chain with the same syndrome may pick another of the tied chains.  A saturated count does not touch the chain."""
    code = _CODES.get(code, code)
    flat, L = _as_chains(code, chains, size)
    c = np.asarray(costs, dtype=np.float64)
    if c.shape != (4,) or not np.all((c >= 0) & (c <= 0xFFFFFFFF) & (c == np.floor(c))):
        raise ValueError(f"costs={costs!r}: the four integer costs of I, X, Y and Z, each >= 0")
    c = c.astype(np.uint32)
    n, ncls = flat.shape[0], 16 if code == L_.TORIC else 4
    out = np.zeros((n, ncls, flat.shape[1]), dtype=np.uint8)
    cost = np.zeros((n, ncls), dtype=np.uint32)
    count = np.zeros((n, ncls), dtype=np.uint64)
    cls = np.zeros(n, dtype=np.int32)
    L_.check(L_.lib().qecmc_class_minplus_chains(code, L, n, L_.u8(flat), c.ctypes.data_as(L_._u32p), int(lds_width), L_.u8(out), cost.ctypes.data_as(L_._u32p),
                                                 count.ctypes.data_as(L_._u64p), L_.i32(cls)))
    info = sweep_cut_info(code, L, lds_width)
    state = (2, L, L) if code in (L_.TORIC, L_.PLANAR) else (L, L)
    return dict(chains=out.reshape((n, ncls) + state), cost=cost, count=count, saturated=count == 0, unique=count == 1, cls=cls, width=info["width"],
                held=info["held"])


def _chains_by_method(code, chains, costs, site_costs, method, size=None, lds_width=0, hbm_width=0, tile_width=0):
    """shortest_chains / shortest_chains_site (method "cut", the default: lds_width) or shortest_chains_tiled / shortest_chains_tiled_site (method
    "tiled", only where it is named: hbm_width, tile_width); a width of the other route is refused by name, as _minplus_by_method refuses it"""
    if method not in _MINPLUS_METHODS:
        raise ValueError(f"method={method!r}: the (min, +) sweep runs on the cut plans ('cut') or tiled over HBM ('tiled')")
    if method == "cut":
        if hbm_width or tile_width:
            raise ValueError("hbm_width and tile_width belong to method='tiled'; method='cut' takes lds_width")
        return shortest_chains(code, chains, costs, size=size, lds_width=lds_width) if site_costs is None else \
            shortest_chains_site(code, chains, site_costs, size=size, lds_width=lds_width)
    if lds_width:
        raise ValueError("lds_width belongs to method='cut'; method='tiled' takes hbm_width and tile_width")
    return shortest_chains_tiled(code, chains, costs, size=size, hbm_width=hbm_width, tile_width=tile_width) if site_costs is None else \
        shortest_chains_tiled_site(code, chains, site_costs, size=size, hbm_width=hbm_width, tile_width=tile_width)


def min_weight_corrections(code, chains, costs=(0, 1, 1, 1), size=None, lds_width=0, method="cut", hbm_width=0, tile_width=0):
    """The minimum-weight decoder's correction: dict(correction uint8[N, ...]: the traced shortest chain (shortest_chains) of target, target int32[N]:
    the class min_weight_classes picks -- the least cost, ties by the larger count, then by the lower class index --, weight uint32[N]: the
    correction's cost, the least of its row).  Nothing with the syndrome of the input is cheaper than the correction.
    method="tiled" traces shortest_chains_tiled's sweep instead (hbm_width, tile_width as it takes them): the shapes past the cut plans."""
    r = _chains_by_method(code, chains, costs, None, method, size=size, lds_width=lds_width, hbm_width=hbm_width, tile_width=tile_width)
    target = _rank_classes(r["cost"], r["count"])
    rows = np.arange(len(target))
    return dict(correction=r["chains"][rows, target], target=target, weight=r["cost"][rows, target])


def _law_from_minplus(cost, count, saturated, base):
    """count * base^(cost - the row's least cost), normalised per row; OverflowError naming the first saturated row"""
    if np.any(saturated):
        row = int(np.flatnonzero(np.any(saturated, axis=1))[0])
        raise OverflowError(f"row {row}: a count of shortest chains passed 2^48 - 1 and is not known (class_minplus reports it as saturated)")
    rel = (cost.astype(np.int64) - cost.astype(np.int64).min(axis=1, keepdims=True)).astype(np.float64)
    z = count.astype(np.float64) * np.power(float(base), rel)
    return z / z.sum(axis=1, keepdims=True)


def shortest_class_law(code, chains, p, alpha=None, site_costs=None, **kw):
    """float64[N, ncls]: the class law carried by the shortest chains alone, count_c * base^cost_c normalised per row (class_minplus, which takes the
    keywords size and lds_width; method="tiled": class_minplus_tiled, which takes size, hbm_width and tile_width) -- computed relative to the row's
    least cost, so nothing underflows.  Depolarizing noise p: unit costs,
    base = (p / 3) / (1 - p).  The alpha model (p is pz_tilde) with an integer-valued alpha: costs (0, alpha, alpha, 1), base = pz_tilde; a
    non-integer alpha raises ValueError.  A row with a saturated count raises OverflowError naming it.
    site_costs (a table as class_minplus_site takes it): count_c * base^cost_c under those costs instead, base formed from p / alpha as above -- the
    caller vouches that the costs are exponents of that base (erasure_site_costs of the noise's own costs are).
    This is the exact value of the second vector of shortest_distribution (unique_n * exp(-beta * shortest), there in percent) once its ladder has
    seen every shortest chain of every class, and the low-p limit of exact_class_probabilities."""
    if alpha is None:
        costs, base = (0, 1, 1, 1), (p / 3.0) / (1.0 - p)
    else:
        if float(alpha) != np.floor(float(alpha)) or not 0 <= float(alpha) <= 255:
            raise ValueError(f"alpha={alpha!r}: shortest_class_law takes integer costs, so an integer-valued alpha in 0 .. 255 (non-integer costs are out of scope)")
        costs, base = (0, int(alpha), int(alpha), 1), float(p)
    r = _minplus_by_method(code, chains, costs, site_costs, kw.pop("method", "cut"), **kw)
    return _law_from_minplus(r["cost"], r["count"], r["saturated"], base)


def _as_site_costs(code, site_costs, L, n):
    """site_costs -> (uint8[rows, nq, 4], rows): integers 0 .. 255 shaped as _as_site_weights takes its weights; ValueError naming the first cell that is
    no such integer"""
    a = np.asarray(site_costs)
    if a.dtype.kind not in "biuf":
        raise ValueError(f"site_costs of dtype {a.dtype}: integer costs 0 .. 255")
    try:
        wq, rows = _as_site_weights(code, a.astype(np.float64), L, n)
    except ValueError as e:
        raise ValueError(str(e).replace("site_weights", "site_costs")) from None
    bad = ~(np.isfinite(wq) & (wq >= 0) & (wq <= 255) & (wq == np.floor(np.where(np.isfinite(wq), wq, 0.0))))
    if bad.any():
        r, q, i = (int(x) for x in np.argwhere(bad)[0])
        raise ValueError(f"site_costs[row {r}][qubit {q}][{'IXYZ'[i]}]={float(wq[r, q, i])!r}: the site costs are integers 0 .. 255")
    return np.ascontiguousarray(wq.astype(np.uint8)), rows


def class_minplus_site(code, chains, site_costs, size=None, lds_width=0):
    """class_minplus under a cost per qubit, or per (syndrome, qubit), on the GPU (qecmc_class_minplus_site).  code, chains, size and
    lds_width as class_minplus takes them.  site_costs: integer [..., 4], the costs of I, X, Y and Z at every cell of the state layout, 0 .. 255 each,
    ... being the code's qubit_matrix shape or the flat nq; one table for all syndromes (alone or after a leading 1), or with a leading N one per
    syndrome.  The planar code's unused cells are not read.  erasure_site_costs and llr_site_costs build such tables.
    Returns class_minplus's dict, key for key: cost[s, c] the least sum over the qubits of site_costs[row(s), q, Pauli at q]."""
    code = _CODES.get(code, code)
    flat, L = _as_chains(code, chains, size)
    n, ncls = flat.shape[0], 16 if code == L_.TORIC else 4
    cq, rows = _as_site_costs(code, site_costs, L, n)
    cost = np.zeros((n, ncls), dtype=np.uint32)
    count = np.zeros((n, ncls), dtype=np.uint64)
    cls = np.zeros(n, dtype=np.int32)
    L_.check(L_.lib().qecmc_class_minplus_site(code, L, n, L_.u8(flat), L_.u8(cq), rows, int(lds_width), cost.ctypes.data_as(L_._u32p),
                                               count.ctypes.data_as(L_._u64p), L_.i32(cls)))
    info = sweep_cut_info(code, L, lds_width)
    return dict(cost=cost, count=count, saturated=count == 0, cls=cls, width=info["width"], held=info["held"])


def shortest_chains_site(code, chains, site_costs, size=None, lds_width=0):
    """shortest_chains under a cost per qubit, or per (syndrome, qubit), on the GPU (qecmc_class_minplus_chains_site): the arguments
    are class_minplus_site's, the dict is shortest_chains', key for key -- chains[s, c] has the syndrome of chain s, lies in class c and costs
    cost[s, c] under the table.  Under llr_site_costs it is a most likely chain of its class, exactly; where unique, THE most likely one."""
    code = _CODES.get(code, code)
    flat, L = _as_chains(code, chains, size)
    n, ncls = flat.shape[0], 16 if code == L_.TORIC else 4
    cq, rows = _as_site_costs(code, site_costs, L, n)
    out = np.zeros((n, ncls, flat.shape[1]), dtype=np.uint8)
    cost = np.zeros((n, ncls), dtype=np.uint32)
    count = np.zeros((n, ncls), dtype=np.uint64)
    cls = np.zeros(n, dtype=np.int32)
    L_.check(L_.lib().qecmc_class_minplus_chains_site(code, L, n, L_.u8(flat), L_.u8(cq), rows, int(lds_width), L_.u8(out), cost.ctypes.data_as(L_._u32p),
                                                      count.ctypes.data_as(L_._u64p), L_.i32(cls)))
    info = sweep_cut_info(code, L, lds_width)
    state = (2, L, L) if code in (L_.TORIC, L_.PLANAR) else (L, L)
    return dict(chains=out.reshape((n, ncls) + state), cost=cost, count=count, saturated=count == 0, unique=count == 1, cls=cls, width=info["width"],
                held=info["held"])


def min_weight_classes_site(code, chains, site_costs, size=None, lds_width=0, method="cut", hbm_width=0, tile_width=0):
    """int32[N]: min_weight_classes under site costs -- the class class_minplus_site (method="tiled": class_minplus_tiled_site) gives the least cost,
    ties broken by the larger count, then by the lower class index"""
    r = _minplus_by_method(code, chains, None, site_costs, method, size=size, lds_width=lds_width, hbm_width=hbm_width, tile_width=tile_width)
    return _rank_classes(r["cost"], r["count"])


def min_weight_corrections_site(code, chains, site_costs, size=None, lds_width=0, method="cut", hbm_width=0, tile_width=0):
    """min_weight_corrections under site costs: dict(correction: the traced shortest chain (shortest_chains_site; method="tiled":
    shortest_chains_tiled_site) of target, target: the class min_weight_classes_site picks, weight uint32[N]: the correction's cost under the table,
    the least of its row)"""
    r = _chains_by_method(code, chains, None, site_costs, method, size=size, lds_width=lds_width, hbm_width=hbm_width, tile_width=tile_width)
    target = _rank_classes(r["cost"], r["count"])
    rows = np.arange(len(target))
    return dict(correction=r["chains"][rows, target], target=target, weight=r["cost"][rows, target])


def erasure_site_costs(base_costs, erased):
    """site costs of a batch of shots with erasures: uint8[erased.shape + (4,)].  base_costs: the integer costs off the erased sets, [4] (one for all
    cells) or [..., 4]; erased: a bool mask [N, ...] or [...].  An erased cell carries a uniform Pauli, so nothing there tells one chain from another:
    it gets (0, 0, 0, 0)."""
    erased = np.asarray(erased, dtype=bool)
    base = np.asarray(base_costs)
    if base.dtype.kind not in "biuf" or not np.all(np.isfinite(base)) or not np.all((base >= 0) & (base <= 255) & (base == np.floor(base))):
        raise ValueError("base_costs: integer costs 0 .. 255")
    out = np.array(np.broadcast_to(base.astype(np.uint8), erased.shape + (4,)))
    out[erased] = 0
    return out


def llr_site_costs(site_w4, scale):
    """integer log-likelihood costs of site weights: uint8[...], cost[q][P] = rint(scale * ln(max_P' w_q[P'] / w_q[P])) for site_w4 float [..., 4] (as the
    _site_w4 builders return it), so that the likeliest Pauli of a cell costs 0 and the shortest chain under the table is the most likely one on the
    scale's grid.  Weights that are exact powers base^k of one base give k at scale = 1 / ln(1 / base).  ValueError naming the first cell with a
    zero, negative or non-finite weight, or whose cost passes 255: there is no silent cap."""
    w = np.asarray(site_w4, dtype=np.float64)
    if w.ndim < 1 or w.shape[-1] != 4:
        raise ValueError(f"site_w4 of shape {w.shape}: [..., 4], the weights of I, X, Y and Z per cell")
    bad = ~(np.isfinite(w) & (w > 0))
    if bad.any():
        cell = tuple(int(x) for x in np.argwhere(bad)[0])
        raise ValueError(f"site_w4{list(cell[:-1])}[{'IXYZ'[cell[-1]]}]={float(w[cell])!r}: llr_site_costs takes finite weights > 0 (an erased cell is (1, 1, 1, 1), a cost of 0)")
    if not np.isfinite(scale) or not scale > 0:
        raise ValueError(f"scale={scale!r}: a finite number > 0")
    cost = np.rint(float(scale) * (np.log(w.max(axis=-1, keepdims=True)) - np.log(w)))
    if (cost > 255).any():
        cell = tuple(int(x) for x in np.argwhere(cost > 255)[0])
        raise ValueError(f"site_w4{list(cell[:-1])}[{'IXYZ'[cell[-1]]}]: a cost of {int(cost[cell])} at scale {scale!r} passes 255; lower the scale")
    return cost.astype(np.uint8)


def sweep_tiled_info(code, size, hbm_width=0, tile_width=0):
    """dict(full_width, width, held, ncls, nq, n_ops, segments) of the tiled plan of one (code, size) for a state vector of at most 2^hbm_width
    doubles in HBM and tiles of 2^tile_width doubles in LDS (0: the library's defaults, 24 and 11), from the host half of the library alone; raises
    QecmcError where the plan is refused"""
    v = [C.c_int32() for _ in range(7)]
    L_.check(L_.lib().qecmc_class_sweep_tiled_info(_CODES.get(code, code), int(size), int(hbm_width), int(tile_width), *[C.byref(x) for x in v]))
    return dict(zip(("full_width", "width", "held", "ncls", "nq", "n_ops", "segments"), (int(x.value) for x in v)))


def class_sweep_tiled(code, chains, weights, size=None, hbm_width=0, tile_width=0):
    """class_sweep on a state vector tiled over HBM (qecmc_class_sweep_tiled): xzzx / rotated L = 13 .. 21, planar L = 8 .. 12 and,
    with `held` generators held out as class_sweep_cut holds them, the toric code at L = 7.  hbm_width: the widest state vector, tile_width .. 24
    (2^24 doubles are 128 MiB per class and assignment), 0: the default; tile_width: the index bits of a tile in LDS, 4 .. 13, 0: the default.  The
    result does not depend on tile_width, bit for bit.
    Returns dict(Z float64[N, ncls], cls int32[N], width: the widest frontier of the plan, held: the number of held generators, segments: the launches
    one pass of state vectors takes).  Z is raw, as class_sweep's: it may be subnormal, 0 or inf, and law_from_class_weights is where that is judged."""
    code = _CODES.get(code, code)
    flat, L = _as_chains(code, chains, size)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (4,):
        raise ValueError(f"weights of shape {w.shape}: the four weights of I, X, Y and Z")
    info = sweep_tiled_info(code, L, hbm_width, tile_width)
    n = flat.shape[0]
    z = np.zeros((n, info["ncls"]), dtype=np.float64)
    cls = np.zeros(n, dtype=np.int32)
    f64p = C.POINTER(C.c_double)
    L_.check(L_.lib().qecmc_class_sweep_tiled(code, L, n, L_.u8(flat), w.ctypes.data_as(f64p), int(hbm_width), int(tile_width), z.ctypes.data_as(f64p),
                                              L_.i32(cls)))
    return dict(Z=z, cls=cls, width=info["width"], held=info["held"], segments=info["segments"])


def class_minplus_tiled(code, chains, costs=(0, 1, 1, 1), size=None, hbm_width=0, tile_width=0):
    """class_minplus on the state vector tiled over HBM (qecmc_class_minplus_tiled): the least cost of every class and the number of
    chains that reach it at xzzx / rotated L = 13 .. 21, planar L = 8 .. 12 and the toric code at L = 7 -- class_sweep_tiled's plans in the semiring of
    (cost, count) pairs.  code, chains and costs as class_minplus takes them, hbm_width and tile_width as class_sweep_tiled's; the result does not depend
    on tile_width.  The costs must keep a chain's cost below 2^16: n_qubits * max(costs) < 65536, refused by name otherwise.  shortest_chains_tiled
    traces a chain back.
    Returns class_minplus's dict, key for key -- cost uint32[N, ncls], count uint64[N, ncls], saturated bool[N, ncls], cls int32[N], width, held: the
    tiled plan's -- plus segments: the launches one pass of state vectors takes."""
    code = _CODES.get(code, code)
    flat, L = _as_chains(code, chains, size)
    c = np.asarray(costs, dtype=np.float64)
    if c.shape != (4,) or not np.all((c >= 0) & (c <= 0xFFFFFFFF) & (c == np.floor(c))):
        raise ValueError(f"costs={costs!r}: the four integer costs of I, X, Y and Z, each >= 0")
    c = c.astype(np.uint32)
    n, ncls = flat.shape[0], 16 if code == L_.TORIC else 4
    cost = np.zeros((n, ncls), dtype=np.uint32)
    count = np.zeros((n, ncls), dtype=np.uint64)
    cls = np.zeros(n, dtype=np.int32)
    L_.check(L_.lib().qecmc_class_minplus_tiled(code, L, n, L_.u8(flat), c.ctypes.data_as(L_._u32p), int(hbm_width), int(tile_width), cost.ctypes.data_as(L_._u32p),
                                                count.ctypes.data_as(L_._u64p), L_.i32(cls)))
    info = sweep_tiled_info(code, L, hbm_width, tile_width)
    return dict(cost=cost, count=count, saturated=count == 0, cls=cls, width=info["width"], held=info["held"], segments=info["segments"])


def class_minplus_tiled_site(code, chains, site_costs, size=None, hbm_width=0, tile_width=0):
    """class_minplus_tiled under a cost per qubit, or per (syndrome, qubit) (qecmc_class_minplus_tiled_site): site_costs as
    class_minplus_site takes them, the widths as class_minplus_tiled's.  Every row must keep a chain's cost below 2^16: the sum over the qubits of the
    row's largest cost at the qubit < 65536, refused otherwise with the row named.  Returns class_minplus_tiled's dict, key for key."""
    code = _CODES.get(code, code)
    flat, L = _as_chains(code, chains, size)
    n, ncls = flat.shape[0], 16 if code == L_.TORIC else 4
    cq, rows = _as_site_costs(code, site_costs, L, n)
    cost = np.zeros((n, ncls), dtype=np.uint32)
    count = np.zeros((n, ncls), dtype=np.uint64)
    cls = np.zeros(n, dtype=np.int32)
    L_.check(L_.lib().qecmc_class_minplus_tiled_site(code, L, n, L_.u8(flat), L_.u8(cq), rows, int(hbm_width), int(tile_width), cost.ctypes.data_as(L_._u32p),
                                                     count.ctypes.data_as(L_._u64p), L_.i32(cls)))
    info = sweep_tiled_info(code, L, hbm_width, tile_width)
    return dict(cost=cost, count=count, saturated=count == 0, cls=cls, width=info["width"], held=info["held"], segments=info["segments"])


def shortest_chains_tiled(code, chains, costs=(0, 1, 1, 1), size=None, hbm_width=0, tile_width=0):
    """shortest_chains on the state vector tiled over HBM (qecmc_class_minplus_tiled_chains): a shortest chain of every class at xzzx /
    rotated L = 13 .. 21, planar L = 8 .. 12 and the toric code at L = 7 -- class_minplus_tiled's sweep traced back.  The arguments are
    class_minplus_tiled's.  Returns shortest_chains' dict -- chains uint8[N, ncls, ...], cost, count, saturated, unique, cls, width, held: the tiled
    plan's -- plus segments.  The chain obeys shortest_chains' tie rule in the plan's own stream: it does not depend on tile_width, and where the
    tiled plan's stream and holds are the cut plan's it is shortest_chains' chain byte for byte."""
    code = _CODES.get(code, code)
    flat, L = _as_chains(code, chains, size)
    c = np.asarray(costs, dtype=np.float64)
    if c.shape != (4,) or not np.all((c >= 0) & (c <= 0xFFFFFFFF) & (c == np.floor(c))):
        raise ValueError(f"costs={costs!r}: the four integer costs of I, X, Y and Z, each >= 0")
    c = c.astype(np.uint32)
    n, ncls = flat.shape[0], 16 if code == L_.TORIC else 4
    out = np.zeros((n, ncls, flat.shape[1]), dtype=np.uint8)
    cost = np.zeros((n, ncls), dtype=np.uint32)
    count = np.zeros((n, ncls), dtype=np.uint64)
    cls = np.zeros(n, dtype=np.int32)
    L_.check(L_.lib().qecmc_class_minplus_tiled_chains(code, L, n, L_.u8(flat), c.ctypes.data_as(L_._u32p), int(hbm_width), int(tile_width), L_.u8(out),
                                                       cost.ctypes.data_as(L_._u32p), count.ctypes.data_as(L_._u64p), L_.i32(cls)))
    info = sweep_tiled_info(code, L, hbm_width, tile_width)
    state = (2, L, L) if code in (L_.TORIC, L_.PLANAR) else (L, L)
    return dict(chains=out.reshape((n, ncls) + state), cost=cost, count=count, saturated=count == 0, unique=count == 1, cls=cls, width=info["width"],
                held=info["held"], segments=info["segments"])


def shortest_chains_tiled_site(code, chains, site_costs, size=None, hbm_width=0, tile_width=0):
    """shortest_chains_tiled under a cost per qubit, or per (syndrome, qubit) (qecmc_class_minplus_tiled_chains_site): site_costs as
    class_minplus_site takes them, the widths and the cost range as class_minplus_tiled_site's.  Returns shortest_chains_tiled's dict, key for key."""
    code = _CODES.get(code, code)
    flat, L = _as_chains(code, chains, size)
    n, ncls = flat.shape[0], 16 if code == L_.TORIC else 4
    cq, rows = _as_site_costs(code, site_costs, L, n)
    out = np.zeros((n, ncls, flat.shape[1]), dtype=np.uint8)
    cost = np.zeros((n, ncls), dtype=np.uint32)
    count = np.zeros((n, ncls), dtype=np.uint64)
    cls = np.zeros(n, dtype=np.int32)
    L_.check(L_.lib().qecmc_class_minplus_tiled_chains_site(code, L, n, L_.u8(flat), L_.u8(cq), rows, int(hbm_width), int(tile_width), L_.u8(out),
                                                            cost.ctypes.data_as(L_._u32p), count.ctypes.data_as(L_._u64p), L_.i32(cls)))
    info = sweep_tiled_info(code, L, hbm_width, tile_width)
    state = (2, L, L) if code in (L_.TORIC, L_.PLANAR) else (L, L)
    return dict(chains=out.reshape((n, ncls) + state), cost=cost, count=count, saturated=count == 0, unique=count == 1, cls=cls, width=info["width"],
                held=info["held"], segments=info["segments"])


def class_weights(hist, weight):
    """Z[..., c] = sum over (n_xy, n_z) of hist[..., c, n_xy, n_z] * weight(n_xy, n_z): weight is broadcast over the grid of counts, float64"""
    hist = np.asarray(hist)
    n = np.arange(hist.shape[-1], dtype=np.float64)
    w = np.broadcast_to(np.asarray(weight(n[:, None], n[None, :]), dtype=np.float64), hist.shape[-2:])
    return np.einsum("...ij,ij->...", hist.astype(np.float64), w)


def depolarizing_weight(p):
    """f^(n_xy + n_z), f = (p / 3) / (1 - p)"""
    f = (p / 3.0) / (1.0 - p)
    return lambda nxy, nz: f ** (nxy + nz)


def biased_weight(p, eta):
    """(p_x / p_I)^n_xy (p_z / p_I)^n_z with p_z = p eta / (eta + 1), p_x = p_y = p / (2 (eta + 1)), p_I = 1 - p: the ratio form, so a cell that holds
    no qubit (the planar code's) does not enter"""
    rz, rx = p * eta / (eta + 1.0) / (1.0 - p), p / (2.0 * (eta + 1.0)) / (1.0 - p)
    return lambda nxy, nz: rx ** nxy * rz ** nz


def alpha_weight(pz_tilde, alpha):
    """pz_tilde^(n_z + alpha n_xy)"""
    return lambda nxy, nz: pz_tilde ** (nz + alpha * nxy)


def depolarizing_w4(p):
    """depolarizing_weight per qubit: (1, f, f, f), f = (p / 3) / (1 - p)"""
    f = (p / 3.0) / (1.0 - p)
    return np.array([1.0, f, f, f])


def biased_w4(p, eta):
    """biased_weight per qubit: (1, p_x / p_I, p_y / p_I, p_z / p_I)"""
    rz, rx = p * eta / (eta + 1.0) / (1.0 - p), p / (2.0 * (eta + 1.0)) / (1.0 - p)
    return np.array([1.0, rx, rx, rz])


def alpha_w4(pz_tilde, alpha):
    """alpha_weight per qubit: (1, pz_tilde^alpha, pz_tilde^alpha, pz_tilde)"""
    return np.array([1.0, pz_tilde ** alpha, pz_tilde ** alpha, pz_tilde])


_SITE_METHODS = ("auto", "sweep", "cut", "tiled")


def _as_site_weights(code, site_weights, L, n):
    """site_weights -> (float64[rows, nq, 4], rows): [..., 4] with ... the code's qubit_matrix shape or the flat nq, with or without a leading N"""
    a = np.ascontiguousarray(site_weights, dtype=np.float64)
    matrix = (2, L, L) if code in (L_.TORIC, L_.PLANAR) else (L, L)
    nq = int(np.prod(matrix))
    if a.ndim >= 2 and a.shape[-1] == 4:
        if a.shape[:-1] in (matrix, (nq,)):
            return a.reshape(1, nq, 4), 1
        if a.shape[0] in (1, n) and a.shape[1:-1] in (matrix, (nq,)):           # (a leading 1 is one table for every syndrome)
            return a.reshape(a.shape[0], nq, 4), a.shape[0]
    raise ValueError(f"site_weights of shape {a.shape}: [..., 4] with ... = {matrix} or ({nq},), alone or after a leading 1 or N = {n}")


def resolve_site_method(code, size, method="auto", lds_width=0, hbm_width=0, tile_width=0):
    """(method, info) class_sweep_site runs at one (code, size): the method named, or for "auto" the first of "sweep", "cut", "tiled" whose _info call
    accepts the shape, with that plan's dict(width, held, ncls, nq, ...).  Unlike resolve_method, "auto" does reach "tiled": class_sweep_site has no
    earlier answer to preserve.  Where every route refuses, the QecmcError raised is the last one's -- the tiled sweep's, which reaches furthest.
    From the host half of the library alone."""
    if method not in _SITE_METHODS:
        raise ValueError(f"method={method!r}: class_sweep_site runs {_SITE_METHODS[1:]} or 'auto'")
    code = _CODES.get(code, code)
    infos = {"sweep": lambda: dict(sweep_info(code, size), held=0), "cut": lambda: sweep_cut_info(code, size, lds_width),
             "tiled": lambda: sweep_tiled_info(code, size, hbm_width, tile_width)}
    for m in (_SITE_METHODS[1:] if method == "auto" else (method,)):
        try:
            return m, infos[m]()
        except L_.QecmcError as e:
            refusal = e
    raise refusal


def class_sweep_site(code, chains, site_weights, size=None, method="auto", lds_width=0, hbm_width=0, tile_width=0):
    """The class weights of every syndrome under a weight per qubit, or per (syndrome, qubit), on the GPU (qecmc_class_sweep_site, _cut_site,
    _tiled_site).  code and chains as class_sweep takes them.  site_weights: float [..., 4], the weights of I, X, Y and Z at every cell
    of the state layout, ... being the code's qubit_matrix shape or the flat nq; one table for all syndromes, or with a leading N one per syndrome.
    Weights are finite and >= 0 -- zero is allowed, a qubit whose four weights are all zero is not; the planar code's unused cells are not read.
    method: "sweep", "cut" (lds_width), "tiled" (hbm_width, tile_width) or "auto": the first of sweep, cut, tiled whose plan is accepted
    (resolve_site_method).  This "auto" does reach the tiled sweep -- unlike exact_class_probabilities, whose routing is kept as it was: there is no
    earlier answer to preserve here.
    Returns dict(Z float64[N, ncls]: Z[s, c] = the sum over the chains of class c with the syndrome of chain s of the product over the qubits of the
    weight of their Pauli there, cls int32[N], method: the one that ran, width, held).  Z is raw: with weights above 1 it may reach inf, with small
    ones the subnormals or 0; law_from_class_weights (exact_site_probabilities) is where that is judged."""
    code = _CODES.get(code, code)
    if method not in _SITE_METHODS:
        raise ValueError(f"method={method!r}: class_sweep_site runs {_SITE_METHODS[1:]} or 'auto'")
    flat, L = _as_chains(code, chains, size)
    n = flat.shape[0]
    wq, rows = _as_site_weights(code, site_weights, L, n)
    ran, info = resolve_site_method(code, L, method, lds_width, hbm_width, tile_width)
    z = np.zeros((n, info["ncls"]), dtype=np.float64)
    cls = np.zeros(n, dtype=np.int32)
    f64p = C.POINTER(C.c_double)
    head = (code, L, n, L_.u8(flat), wq.ctypes.data_as(f64p), rows)
    tail = (z.ctypes.data_as(f64p), L_.i32(cls))
    if ran == "sweep":
        L_.check(L_.lib().qecmc_class_sweep_site(*head, *tail))
    elif ran == "cut":
        L_.check(L_.lib().qecmc_class_sweep_cut_site(*head, int(lds_width), *tail))
    else:
        L_.check(L_.lib().qecmc_class_sweep_tiled_site(*head, int(hbm_width), int(tile_width), *tail))
    return dict(Z=z, cls=cls, method=ran, width=info["width"], held=info["held"])


# The least row total law_from_class_weights normalises.  The sweeps and the enumerator's sum work in ratio form with no rescaling, so a class weight
# is about count * f^cost and leaves the normal range of float64 at low p and large L.  Below 2^-1022 every product and sum rounds to a multiple of
# 2^-1074, an absolute error of at most 2^-1075 each.  The largest accepted plan performs fewer than 2^46 additions per output (2^24 entries of the
# tiled state vector x about 10^3 ops x 2^12 held assignments), so a class weight is off by less than 2^46 * 2^-1075 = 2^-1029 absolute whatever the
# route, and a law to 1e-12 (about 2^-40) needs a total above 2^-989.  2^-960 leaves a factor 2^29 over that crude bound.  The comparison is made at
# half of it, so that a row whose exact total is 2^-960 or more is never refused on account of the sweep's own relative error.
LAW_FLOOR = 2.0 ** -961
_ALL_ZERO = "every class weight of a syndrome underflows to 0 in float64: the law of that row is not representable"


def law_from_class_weights(z):
    """float64[..., ncls]: class weights Z normalised per row -- the one place where the range of a sweep's raw Z is judged.  Raises
    FloatingPointError naming the first offending row and the end of float64's range it met: a class weight (or the row's total) that is not finite
    -- overflow, weights above 1 --, or a row total below 2^-960 (LAW_FLOOR, compared at half of it) -- underflow: its class weights were rounded in the subnormal range, or
    to 0, and their ratios are no longer the law.  A class that underflows to 0 beside a total >= LAW_FLOOR stays: its probability is below 2^-60."""
    z = np.asarray(z, dtype=np.float64)
    rows = z.reshape(-1, z.shape[-1])
    with np.errstate(over="ignore", invalid="ignore"):
        tot = rows.sum(axis=1)
    high = ~(np.isfinite(rows).all(axis=1) & np.isfinite(tot))
    low = ~high & ~(tot >= LAW_FLOOR)
    if (high | low).any():
        r = int(np.flatnonzero(high | low)[0])
        if high[r]:
            raise FloatingPointError(f"row {r}: a class weight of the syndrome overflows float64 (class weights {rows[r].tolist()}): weights above 1 took "
                                     "the sweep past the top of the range, and the law of that row is not representable")
        if tot[r] == 0.0:
            raise FloatingPointError(f"{_ALL_ZERO} (row {r}: underflow)")
        raise FloatingPointError(f"row {r}: the class weights of the syndrome total {tot[r]:.3g}, below 2^-960 = {2.0 * LAW_FLOOR:.3g}: they underflow into "
                                 "the subnormal range of float64, where their ratios are rounded away, and the law of that row is not representable")
    return z / tot.reshape(z.shape[:-1] + (1,))


def exact_site_probabilities(code, chains, site_weights, **kw):
    """float64[N, ncls]: the exact class law of every syndrome under site weights -- class_sweep_site's Z, which takes the keywords, normalised per
    row by law_from_class_weights.  Raises FloatingPointError naming the first row whose class weights overflow, or total less than 2^-960 (all 0
    among them), as exact_class_probabilities does."""
    return law_from_class_weights(class_sweep_site(code, chains, site_weights, **kw)["Z"])


def depolarizing_site_w4(p_map):
    """depolarizing_w4 per cell of a map of error rates p_map [...]: float64[..., 4] = (1, f, f, f), f = (p / 3) / (1 - p).  Ratio form: Z differs from
    the Z of the probabilities (1 - p, p / 3, p / 3, p / 3) by the factor prod_q (1 - p_q), common to all classes, so the law is unaffected."""
    p = np.asarray(p_map, dtype=np.float64)
    f = (p / 3.0) / (1.0 - p)
    return np.stack([np.ones_like(f), f, f, f], axis=-1)


def biased_site_w4(p_map, eta):
    """biased_w4 per cell of a map of error rates p_map [...] (eta a number or a map): float64[..., 4] = (1, p_x / p_I, p_y / p_I, p_z / p_I).  Ratio
    form: Z differs from the probability-form Z by the factor prod_q (1 - p_q), common to all classes, so the law is unaffected."""
    p, eta = np.broadcast_arrays(np.asarray(p_map, dtype=np.float64), np.asarray(eta, dtype=np.float64))
    rz, rx = p * eta / (eta + 1.0) / (1.0 - p), p / (2.0 * (eta + 1.0)) / (1.0 - p)
    return np.stack([np.ones_like(rx), rx, rx, rz], axis=-1)


def erasure_site_w4(base_w4, erased):
    """site weights of a batch of shots with erasures: float64[erased.shape + (4,)].  base_w4: the weights off the erased sets, [4] (one for all
    cells) or [..., 4]; erased: a bool mask [N, ...] or [...].  An erased cell carries a uniform Pauli and gets (1, 1, 1, 1).  Ratio form, as
    the builders above: Z differs from the probability-form Z (1 / 4 each on an erased cell) by a factor common to all classes, so the law is
    unaffected."""
    erased = np.asarray(erased, dtype=bool)
    out = np.array(np.broadcast_to(np.asarray(base_w4, dtype=np.float64), erased.shape + (4,)))
    out[erased] = 1.0
    return out


def _sample_w4(p, w4, eta, alpha):
    """the four weights of a sampler call: w4 itself, or the noise model of (p, eta, alpha) as exact_class_probabilities names it"""
    if (w4 is None) == (p is None):
        raise ValueError("give either p (with eta or alpha for the biased / alpha models) or the four weights w4")
    if eta is not None and alpha is not None:
        raise ValueError("eta and alpha name two noise models")
    if w4 is None:
        w4 = alpha_w4(p, alpha) if alpha is not None else biased_w4(p, eta) if eta is not None else depolarizing_w4(p)
    w = np.ascontiguousarray(w4, dtype=np.float64)
    if w.shape != (4,):
        raise ValueError(f"weights of shape {w.shape}: the four weights of I, X, Y and Z")
    return w


def _sample(code, chains, w, site_weights, n_samples, seed, first_syndrome, size, lds_width, mode, tiled=None):
    """both routes: tiled is None on the cut plans (lds_width), or (hbm_width, tile_width, record_bytes) on the plans tiled over HBM"""
    code = _CODES.get(code, code)
    flat, L = _as_chains(code, chains, size)
    n, nq, ncls, K = flat.shape[0], flat.shape[1], 16 if code == L_.TORIC else 4, int(n_samples)
    if not 1 <= K < 2 ** 32:
        raise ValueError(f"n_samples={n_samples!r}: 1 .. 2^32 - 1 samples")
    out = np.zeros((n, K, nq) if mode else (n, ncls, K, nq), dtype=np.uint8)
    cls = np.zeros((n, K), dtype=np.int32)
    z = np.zeros((n, ncls), dtype=np.float64)
    f64p = C.POINTER(C.c_double)
    tail = (K, int(seed), int(first_syndrome), mode, L_.u8(out), L_.i32(cls), z.ctypes.data_as(f64p))
    if tiled is None:
        widths, uniform, site = (int(lds_width),), L_.lib().qecmc_class_sample, L_.lib().qecmc_class_sample_site
    else:
        hbm_width, tile_width, record_bytes = (int(v) for v in tiled)
        if not 0 <= record_bytes < 2 ** 64:
            raise ValueError(f"record_bytes={record_bytes!r}: the cap of the record block in bytes, or 0 for the default")
        widths, uniform, site = (hbm_width, tile_width, record_bytes), L_.lib().qecmc_class_sample_tiled, L_.lib().qecmc_class_sample_tiled_site
    if site_weights is None:
        L_.check(uniform(code, L, n, L_.u8(flat), w.ctypes.data_as(f64p), *widths, *tail))
    else:
        wq, rows = _as_site_weights(code, site_weights, L, n)
        L_.check(site(code, L, n, L_.u8(flat), wq.ctypes.data_as(f64p), rows, *widths, *tail))
    info = sweep_cut_info(code, L, lds_width) if tiled is None else sweep_tiled_info(code, L, widths[0], widths[1])
    state = (2, L, L) if code in (L_.TORIC, L_.PLANAR) else (L, L)
    res = dict(chains=out.reshape(out.shape[:-1] + state), z=z, width=info["width"], held=info["held"])
    if mode:
        res["cls"] = cls
    return res


_SAMPLE_METHODS = ("cut", "tiled")


def _sample_route(method, lds_width, hbm_width, tile_width, record_bytes):
    """the `tiled` argument of _sample for a method: None on the cut plans (the default everywhere), the widths and the cap where "tiled" is named; a
    width of the other route is refused by name, as min_weight_corrections refuses it"""
    if method not in _SAMPLE_METHODS:
        raise ValueError(f"method={method!r}: the exact sampler runs on the cut plans ('cut') or tiled over HBM ('tiled')")
    if method == "cut":
        if hbm_width or tile_width or record_bytes:
            raise ValueError("hbm_width, tile_width and record_bytes belong to method='tiled'; method='cut' takes lds_width")
        return None
    if lds_width:
        raise ValueError("lds_width belongs to method='cut'; method='tiled' takes hbm_width, tile_width and record_bytes")
    return hbm_width, tile_width, record_bytes


def sample_tiled_info(code, size, hbm_width=0, tile_width=0, record_bytes=0):
    """dict(n_forget, bytes_per_job, jobs_per_pass) of the tiled sampler's plan (qecmc_class_sample_tiled_info): the FORGETs of the stream, the bytes one
    job's record takes on the device and the jobs of one record pass under a record block of record_bytes (0: 4 GiB).  A plan whose single job does not
    fit is refused by name with its bytes (QecmcError)"""
    code = _CODES.get(code, code)
    nf, b, j = C.c_int32(), C.c_uint64(), C.c_uint32()
    L_.check(L_.lib().qecmc_class_sample_tiled_info(code, int(size), int(hbm_width), int(tile_width), int(record_bytes), C.byref(nf), C.byref(b), C.byref(j)))
    return dict(n_forget=nf.value, bytes_per_job=b.value, jobs_per_pass=j.value)


def sample_chains_tiled(code, chains, p=None, w4=None, eta=None, alpha=None, n_samples=1, seed=0, first_syndrome=0, size=None, hbm_width=0, tile_width=0,
                        record_bytes=0):
    """sample_chains on the state vector tiled over HBM (qecmc_class_sample_tiled): exact, independent chains of every class at xzzx /
    rotated L = 13 .. 17 under the default record cap -- L = 21, planar L = 8 .. 12 and toric L = 7 under a raised one.  The arguments and the result are
    sample_chains' with lds_width replaced by hbm_width and tile_width as class_sweep_tiled takes them; z is class_sweep_tiled's, bit for bit.
    record_bytes caps the device block of the records (0: 4 GiB; up to 64 GiB): a plan whose single job takes more is refused by name with its bytes
    (QecmcError; sample_tiled_info tells beforehand).  A sample does not depend on tile_width or record_bytes, and where the tiled plan's holds are the
    cut plan's (hbm_width = its lds_width) it is sample_chains' chain byte for byte."""
    return _sample(code, chains, _sample_w4(p, w4, eta, alpha), None, n_samples, seed, first_syndrome, size, 0, 0, tiled=(hbm_width, tile_width, record_bytes))


def sample_chains_tiled_site(code, chains, site_weights, n_samples=1, seed=0, first_syndrome=0, size=None, hbm_width=0, tile_width=0, record_bytes=0):
    """sample_chains_tiled under a weight per qubit, or per (syndrome, qubit) (qecmc_class_sample_tiled_site): site_weights as sample_chains_site takes
    them"""
    return _sample(code, chains, None, site_weights, n_samples, seed, first_syndrome, size, 0, 0, tiled=(hbm_width, tile_width, record_bytes))


def sample_chains(code, chains, p=None, w4=None, eta=None, alpha=None, n_samples=1, seed=0, first_syndrome=0, size=None, lds_width=0):
    """Exact, independent chains of every class of every syndrome, on the GPU (qecmc_class_sample): the cut-set sweep run forward
    with a record and walked back with draws.  code and chains as class_sweep_cut takes them; the weights are w4 -- finite and >= 0, zeros allowed --
    or the noise model of p / (p, eta) / (p as pz_tilde, alpha).  n_samples chains per (syndrome, class).
    Returns dict(chains uint8[N, ncls, n_samples, ...]: chains[s, c, k] has the syndrome of chain s, lies in class c and was drawn with probability
    w(chain) / Z[s, c]; z float64[N, ncls]: class_sweep_cut's Z, bit for bit; width, held).  Sample (s, c, k) is a function of (seed,
    first_syndrome + s, c, k, chain s, the weights) alone: a batch cut into pieces, with first_syndrome moved along, draws the same chains.  A drawn
    chain always has weight > 0, at every range.  A class whose Z is 0, not finite or below 2^-960 (LAW_FLOOR: the record is rounded in the subnormal
    range, and the draws would not follow the law) is refused by row and class (QecmcError)."""
    return _sample(code, chains, _sample_w4(p, w4, eta, alpha), None, n_samples, seed, first_syndrome, size, lds_width, 0)


def sample_chains_site(code, chains, site_weights, n_samples=1, seed=0, first_syndrome=0, size=None, lds_width=0):
    """sample_chains under a weight per qubit, or per (syndrome, qubit) (qecmc_class_sample_site): site_weights as class_sweep_site takes them --
    erasure_site_w4, depolarizing_site_w4, any per-shot prior.  A weight of 0 is never drawn, whatever the range of Z: under erasure_site_w4 with base
    (1, 0, 0, 0) no sample carries an error off the erased set."""
    return _sample(code, chains, None, site_weights, n_samples, seed, first_syndrome, size, lds_width, 0)


def sample_posterior(code, chains, p=None, w4=None, eta=None, alpha=None, site_weights=None, n_samples=1, seed=0, first_syndrome=0, size=None, lds_width=0,
                     method="cut", hbm_width=0, tile_width=0, record_bytes=0):
    """Exact, independent draws from P(chain | syndrome): the class first, with probability Z_c / Z, then a chain of it.  The weights are sample_chains',
    or site_weights as sample_chains_site takes them.
    Returns dict(chains uint8[N, n_samples, ...], cls int32[N, n_samples], z float64[N, ncls], width, held); chains[s, k] is sample_chains' chains[s,
    cls[s, k], k] under the same seed.  A row whose class weights total 0, are not finite, or total less than 2^-960 (LAW_FLOOR) is refused by name
    (QecmcError); a class of weight 0 is never drawn.
    method="tiled" draws on the state vector tiled over HBM instead (sample_chains_tiled; hbm_width, tile_width and record_bytes as it takes them): the
    shapes past the cut plans.  A width of the other route is refused by name."""
    tiled = _sample_route(method, lds_width, hbm_width, tile_width, record_bytes)
    if site_weights is not None:
        if p is not None or w4 is not None:
            raise ValueError("site_weights replace p and w4")
        return _sample(code, chains, None, site_weights, n_samples, seed, first_syndrome, size, lds_width, 1, tiled=tiled)
    return _sample(code, chains, _sample_w4(p, w4, eta, alpha), None, n_samples, seed, first_syndrome, size, lds_width, 1, tiled=tiled)


def posterior_error_counts(code, chains, p, n_samples, seed=0, eta=None, alpha=None, first_syndrome=0, size=None, lds_width=0, method="cut", hbm_width=0, tile_width=0,
                           record_bytes=0):
    """float64[N]: the mean number of errors (cells that hold X, Y or Z) of n_samples exact draws from P(chain | syndrome) at error rate p -- what a
    sampler's rung at p converges to, with an error bar that shrinks as 1 / sqrt(n_samples).  exact_error_counts(...)["posterior"] is the exact value
    this estimates, without draws.  Refused where sample_posterior refuses (QecmcError): a row total of 0, not finite or below 2^-960.
    method, hbm_width, tile_width and record_bytes are sample_posterior's: method="tiled" is the yardstick at the shapes past the cut plans."""
    r = sample_posterior(code, chains, p=p, eta=eta, alpha=alpha, n_samples=n_samples, seed=seed, first_syndrome=first_syndrome, size=size, lds_width=lds_width,
                         method=method, hbm_width=hbm_width, tile_width=tile_width, record_bytes=record_bytes)
    c = r["chains"]
    return (c.reshape(c.shape[0], c.shape[1], -1) != 0).sum(axis=2).mean(axis=1)


def _marginals(code, chains, w, site_weights, size, lds_width):
    code = _CODES.get(code, code)
    flat, L = _as_chains(code, chains, size)
    n, nq, ncls = flat.shape[0], flat.shape[1], 16 if code == L_.TORIC else 4
    weights = np.zeros((n, ncls, nq, 4), dtype=np.float64)
    z = np.zeros((n, ncls), dtype=np.float64)
    cls = np.zeros(n, dtype=np.int32)
    f64p = C.POINTER(C.c_double)
    tail = (int(lds_width), weights.ctypes.data_as(f64p), z.ctypes.data_as(f64p), L_.i32(cls))
    if site_weights is None:
        L_.check(L_.lib().qecmc_class_marginals(code, L, n, L_.u8(flat), w.ctypes.data_as(f64p), *tail))
    else:
        wq, rows = _as_site_weights(code, site_weights, L, n)
        L_.check(L_.lib().qecmc_class_marginals_site(code, L, n, L_.u8(flat), wq.ctypes.data_as(f64p), rows, *tail))
    info = sweep_cut_info(code, L, lds_width)
    state = (2, L, L) if code in (L_.TORIC, L_.PLANAR) else (L, L)
    return dict(weights=weights.reshape((n, ncls) + state + (4,)), z=z, cls=cls, width=info["width"], held=info["held"])


def _judge_range(v, what):
    """The one place where the marginals' raw class weights are judged: v float64[N, ncls] -- every class weight -- or float64[N] -- every row's
    total; what: the quantity asked for.  Raises FloatingPointError naming the first offending row (and class) and the end of float64's range it met,
    in law_from_class_weights' wording: 0 or not finite; or below 2^-960 (LAW_FLOOR, compared at half of it) -- the backward sweep's weights were
    rounded in the subnormal range, and their ratios are no longer the marginals."""
    v = np.asarray(v, dtype=np.float64)
    per_class = v.ndim == 2
    bad = ~(np.isfinite(v) & (v >= LAW_FLOOR))
    if not bad.any():
        return
    at = tuple(int(x) for x in np.argwhere(bad)[0])
    x = float(v[at])
    where = f"row {at[0]}, class {at[1]}: the class weight is" if per_class else f"row {at[0]}: the class weights total"
    if not (np.isfinite(x) and x > 0.0):
        whose = "a class whose weight" if per_class else "a row whose total"
        raise FloatingPointError(f"{where} {x:.3g} -- {whose} is 0 or not finite has no {what}")
    they = "it underflows" if per_class else "they underflow"
    raise FloatingPointError(f"{where} {x:.3g}, below 2^-960 = {2.0 * LAW_FLOOR:.3g}: {they} into the subnormal range of float64, where the ratios of the "
                             f"weights are rounded away, and the {what} of that {'class' if per_class else 'row'} are not representable")


def _normalized(res, normalize):
    """res with marginals = weights / their sum over the last axis; a (row, class) whose class weight _judge_range refuses, or whose four weights total
    0 or are not finite at some qubit, is refused by name.  normalize=False: res as it is, raw -- subnormals, zeros and inf included"""
    w = res["weights"]
    if not normalize:
        return res
    n, ncls = w.shape[:2]
    _judge_range(res["z"], "marginals")
    with np.errstate(over="ignore", invalid="ignore"):
        tot = w.sum(axis=-1)
    bad = ~(np.isfinite(tot) & (tot > 0.0)).reshape(n, ncls, -1).all(axis=2)
    if bad.any():
        r, c = (int(x) for x in np.argwhere(bad)[0])
        raise FloatingPointError(f"row {r}, class {c}: the four weights of a qubit total {float(np.nanmin(tot[r, c])):.3g} at the least (class weight "
                                 f"{float(res['z'][r, c]):.3g}) -- a class whose weight is 0 or not finite has no marginals")
    res["marginals"] = w / tot[..., None]
    return res


def _posterior_of(r, what):
    """float64[N, nq..., 4]: sum_c weights_c / sum_c z_c of a _marginals result, the row total judged by _judge_range"""
    with np.errstate(over="ignore", invalid="ignore"):
        tot = r["z"].sum(axis=1)
        num = r["weights"].sum(axis=1)
    _judge_range(np.where(np.isfinite(num.reshape(len(tot), -1)).all(axis=1), tot, np.inf), what)
    return num / tot.reshape((-1,) + (1,) * (num.ndim - 1))


def class_marginals(code, chains, p=None, w4=None, eta=None, alpha=None, size=None, lds_width=0, normalize=True):
    """The exact marginals of every qubit in every class, on the GPU (qecmc_class_marginals): the cut-set sweep run forward with a
    record of every CLOSE, and a backward sweep over the same stream.  code and chains as class_sweep_cut takes them; the weights are w4 -- finite and
    >= 0, zeros allowed -- or the noise model of p / (p, eta) / (p as pz_tilde, alpha).
    Returns dict(weights float64[N, ncls, ..., 4]: weights[s, c, q, P] = the sum of w(chain) over the chains of class c with the syndrome of chain s
    that carry Pauli P (I, X, Y, Z) at q; marginals = weights / their sum over the last axis (normalize=True): P(q carries P | syndrome, class);
    z float64[N, ncls]: class_sweep_cut's Z, bit for bit; cls int32[N]; width, held).  With normalize=True a (row, class) whose class weight is 0, not
    finite or below 2^-960 (LAW_FLOOR: the weights were rounded in the subnormal range, and their ratios are not the marginals) raises FloatingPointError
    naming row, class and the end of the range it met; at or above 2^-960 the marginals are right to 1e-12.  normalize=False returns the raw weights."""
    return _normalized(_marginals(code, chains, _sample_w4(p, w4, eta, alpha), None, size, lds_width), normalize)


def class_marginals_site(code, chains, site_weights, size=None, lds_width=0, normalize=True):
    """class_marginals under a weight per qubit, or per (syndrome, qubit) (qecmc_class_marginals_site): site_weights as class_sweep_site takes them --
    erasure_site_w4, depolarizing_site_w4, any per-shot prior.  A weight of 0 gives exact zeros: under erasure_site_w4 with base (1, 0, 0, 0) a
    qubit off the erased set carries I with weight z, exactly."""
    return _normalized(_marginals(code, chains, None, site_weights, size, lds_width), normalize)


def posterior_marginals(code, chains, p=None, w4=None, eta=None, alpha=None, site_weights=None, size=None, lds_width=0):
    """float64[N, ..., 4]: P(q carries P | syndrome), the classes mixed with Z_c / Z: sum_c weights_c / sum_c z_c.  The weights are class_marginals',
    or site_weights as class_marginals_site takes them.  A row whose class weights total 0, are not finite, or total less than 2^-960 (LAW_FLOOR) raises
    FloatingPointError naming the row; a class that underflows beside a total above the floor stays: its share is below 2^-60."""
    if site_weights is not None:
        if p is not None or w4 is not None:
            raise ValueError("site_weights replace p and w4")
        r = _marginals(code, chains, None, site_weights, size, lds_width)
    else:
        r = _marginals(code, chains, _sample_w4(p, w4, eta, alpha), None, size, lds_width)
    return _posterior_of(r, "posterior marginals")


def exact_error_counts(code, chains, p, eta=None, alpha=None, size=None, lds_width=0):
    """dict(per_class float64[N, ncls], posterior float64[N]): the exact mean number of errors (cells that hold X, Y or Z) of a chain of class c, and of
    a chain drawn from P(chain | syndrome), at error rate p: sum_q (1 - marginal[q][I]) over the cells that hold a qubit.  posterior is the exact
    value of what posterior_error_counts estimates with n_samples draws.  A class of weight 0, not finite or below 2^-960 is refused by row and class
    (FloatingPointError), as class_marginals refuses it."""
    r = class_marginals(code, chains, p=p, eta=eta, alpha=alpha, size=size, lds_width=lds_width, normalize=True)
    n, ncls = r["z"].shape
    m = r["marginals"].reshape(n, ncls, -1, 4)
    per_class = (1.0 - m[..., 0]).sum(axis=2)                                   # (a cell that holds no qubit carries the representative's I: 1 - 1)
    post = _posterior_of(r, "posterior").reshape(n, -1, 4)
    return dict(per_class=per_class, posterior=(1.0 - post[..., 0]).sum(axis=1))


_METHODS = ("auto", "enumerate", "sweep", "cut", "tiled")


def resolve_method(code, size, method="auto"):
    """what exact_class_probabilities runs at one (code, size): "auto" is the enumerator wherever it accepts the shape -- so a call that worked
    before the sweep existed returns what it returned --, the sweep where the enumerator answers QECMC_ERR_UNSUPPORTED, and the cut-set sweep where
    the sweep answers QECMC_ERR_UNSUPPORTED too and the cut plan is accepted; any other answer is the enumerator's to report.  "auto" never answers
    "tiled": the sweep tiled over HBM runs only where it is named, and where all three refuse the refusal a caller sees is still the sweep's.  From
    the host half of the library alone."""
    if method not in _METHODS:
        raise ValueError(f"method={method!r}")
    if method != "auto":
        return method
    code = _CODES.get(code, code)
    if L_.lib().qecmc_coset_enumerate_info(code, int(size), None, None, None, None) != -4:
        return "enumerate"
    if L_.lib().qecmc_class_sweep_info(code, int(size), None, None, None, None) == -4 and \
            L_.lib().qecmc_class_sweep_cut_info(code, int(size), 0, None, None, None, None, None, None) == 0:
        return "cut"
    return "sweep"


def exact_class_probabilities(code, chains, p, eta=None, alpha=None, hist=None, method="auto", **enumerator_kw):
    """float64[N, ncls]: the exact class law of every syndrome under depolarizing noise p, Z-biased noise (p, eta) or the alpha model (p is pz_tilde).
    method "enumerate": by coset_enumerator, which takes the keywords; "sweep": by class_sweep (of the keywords it takes size and device; chunk_bits
    means nothing to it); "cut": by class_sweep_cut (size, and lds_width); "auto" (default): the enumerator wherever it accepts the (code, size), the
    sweep where it does not, the cut-set sweep where neither does; "tiled": by class_sweep_tiled (size, hbm_width and tile_width), which "auto"
    never picks.
    hist: a histogram already enumerated (coset_enumerator(...)['hist']) -- chains is then not looked at, and the method is the enumerator's.
    Range: the class weights are formed in ratio form (1, f, f, f) with no rescaling, about count * f^cost; law_from_class_weights normalises them and
    raises FloatingPointError naming the first row whose weights overflow or total less than 2^-960 (about 1e-289) -- right, or refused by name."""
    if eta is not None and alpha is not None:
        raise ValueError("eta and alpha name two noise models")
    if method not in _METHODS:
        raise ValueError(f"method={method!r}")
    if hist is None:
        method = resolve_method(code, _as_chains(_CODES.get(code, code), chains, enumerator_kw.get("size"))[1], method)
    if hist is None and method in ("sweep", "cut", "tiled"):
        if "chunks" in enumerator_kw:
            raise ValueError("chunks= is the enumerator's: the sweep has no partial sums")
        w4 = alpha_w4(p, alpha) if alpha is not None else biased_w4(p, eta) if eta is not None else depolarizing_w4(p)
        if method in ("cut", "tiled") and int(enumerator_kw.get("device", 0)) != 0:
            raise ValueError(f"class_sweep_{method} runs on device 0: the library has no device-pointer form of it yet")
        if method == "tiled":
            z = class_sweep_tiled(code, chains, w4, size=enumerator_kw.get("size"), hbm_width=enumerator_kw.get("hbm_width", 0),
                                  tile_width=enumerator_kw.get("tile_width", 0))["Z"]
        elif method == "cut":
            z = class_sweep_cut(code, chains, w4, size=enumerator_kw.get("size"), lds_width=enumerator_kw.get("lds_width", 0))["Z"]
        else:
            z = class_sweep(code, chains, w4, size=enumerator_kw.get("size"), device=enumerator_kw.get("device", 0))["Z"]
    else:
        if hist is None:
            hist = coset_enumerator(code, chains, **enumerator_kw)["hist"]
        weight = alpha_weight(p, alpha) if alpha is not None else biased_weight(p, eta) if eta is not None else depolarizing_weight(p)
        z = class_weights(hist, weight)
    return law_from_class_weights(z)


def exact_rung_observables(hist, p_ladder):
    """float64[N, Nc]: the exact mean error count of every rung of a depolarizing ladder (np.linspace(p, 0.75, Nc) in the decoders).  A rung samples
    f_rung^n over the union of the classes: the truth of nerr_sums / steps."""
    tot = np.asarray(hist).sum(axis=-3).astype(np.float64)                     # [N, n_xy, n_z]
    n = np.arange(tot.shape[-1], dtype=np.float64)
    errs = n[:, None] + n[None, :]
    out = []
    for p in np.atleast_1d(np.asarray(p_ladder, dtype=np.float64)):
        w = ((p / 3.0) / (1.0 - p)) ** errs
        out.append(np.einsum("...ij,ij->...", tot, w * errs) / np.einsum("...ij,ij->...", tot, w))
    return np.stack(out, axis=-1)
