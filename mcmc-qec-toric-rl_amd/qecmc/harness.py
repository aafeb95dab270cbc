"""Batched counterpart of the reference's data-generation harness (`generate_data.generate`,
generate_data.py:20-269).

The reference makes one random error, hides its class with a random logical operator, decodes it
with one `PTEQ` call and appends (qubit_matrix, distribution) to a pandas pickle, one syndrome at a
time.  Here the seed configurations of a whole batch are drawn on the host (NumPy, the recipe of
toric_model.py:15-24 / xzzx_model.py:16-30 and generate_data.py:121-131), decoded in ONE batched
GPU call, and returned / saved as plain arrays (npz instead of the MultiIndex pickle).
"""
import numpy as np

from . import _lib as L_
from .decoders import (nall_n_alpha_distribution, pteq_batch, ptdc_batch, ptdc_distribution, ptrc_distribution,
                       strc_distribution)

_CODES = {"toric": L_.TORIC, "xzzx": L_.XZZX, "rotated": L_.ROTATED, "planar": L_.PLANAR}


def _class_of(code, m):
    from . import _surf, planar_model, toric_model
    if code == L_.PLANAR:
        return planar_model.eq_class(m)
    return toric_model.eq_class(m) if code == L_.TORIC else _surf.eq_class(code, m)


def alpha_rates(pz_tilde, alpha):
    """(p_x, p_y, p_z) of the alpha noise model (generate_data.py:84-91, mcmc_alpha.py:31-36)."""
    p_tilde = pz_tilde + 2 * pz_tilde ** alpha
    p = p_tilde / (1 + p_tilde)
    px = pz_tilde ** alpha * (1 - p)
    return px, px, pz_tilde * (1 - p)


def biased_as_alpha(p, eta):
    """generate_data.py:145-146: the (pz_tilde, alpha) that `generate` hands to PTEQ_alpha for noise = 'biased'."""
    pz_tilde = (p / (1 + 1 / eta)) / (1 - p)
    return pz_tilde, np.log(pz_tilde / (2 * eta)) / np.log(pz_tilde)


def draw_errors(code, size, n, p_error, rng, eta=None, rates=None):
    """n random error chains: toric -- each qubit errs w.p. p_error, Pauli uniform (toric_model.py:15-23);
    xzzx / rotated -- one uniform per qubit against (p_z, p_x, p_y) (xzzx_model.py:16-30), with
    p_x = p_y = p_z = p/3 (generate_data.py:116-118) or the Z-biased split p_z = p eta/(eta+1),
    p_x = p_y = p/(2(eta+1)) (generate_data.py:78-83)."""
    code = _CODES.get(code, code)
    if code == L_.TORIC:
        m = np.zeros((n, 2, size, size), dtype=np.uint8)
        err = rng.random(m.shape) < p_error
        m[err] = rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)
        return m
    if rates is not None:
        px, py, pz = rates
    elif eta is None:
        px = py = pz = p_error / 3
    else:
        pz, px = p_error * eta / (eta + 1), p_error / (2 * (eta + 1))
        py = px
    shape = (n, 2, size, size) if code == L_.PLANAR else (n, size, size)
    r = rng.random(shape)
    m = np.zeros(shape, dtype=np.uint8)
    m[r < pz] = 3
    m[(r > pz) & (r < pz + px)] = 1
    m[(r > pz + px) & (r < pz + px + py)] = 2
    if code == L_.PLANAR:                 # layer 1 lives on its first L-1 rows / columns (planar_model.py:38-39)
        m[:, 1, -1, :] = 0
        m[:, 1, :, -1] = 0
    return m


def generate_syndromes(code, size, n, p_error=None, eta=None, rates=None, hide=True, seed=0, first_syndrome=0):
    """The generation half of the recipe ON THE DEVICE (qecmc_generate_syndromes): n error chains by the model's
    generate_random_error, their equivalence class, and -- hide=True -- one apply_random_logical on top (generate_data.py:110-131).
    Rates as in draw_errors: toric / depolarizing p_x = p_y = p_z = p_error / 3, the Z-biased split for eta, or explicit `rates`.
    Syndrome s draws from Philox (seed, first_syndrome + s).  Returns (init uint8[n, ...], raw uint8[n, ...], eq_true int32[n])."""
    code = _CODES.get(code, code)
    if rates is not None:
        px, py, pz = rates
    elif eta is None or code == L_.TORIC:
        px = py = pz = p_error / 3
    else:
        pz, px = p_error * eta / (eta + 1), p_error / (2 * (eta + 1))
        py = px
    shape = (n, 2, size, size) if code in (L_.TORIC, L_.PLANAR) else (n, size, size)
    init = np.zeros(shape, dtype=np.uint8)
    raw = np.zeros(shape, dtype=np.uint8)
    eq = np.zeros(n, dtype=np.int32)
    L_.check(L_.lib().qecmc_generate_syndromes(code, size, n, float(px), float(py), float(pz), int(bool(hide)), seed & 0xFFFFFFFFFFFFFFFF,
                                               first_syndrome, L_.u8(init), L_.u8(raw), L_.i32(eq)))
    return init, raw, eq


def hide_class(code, m, rng):
    """`init_code.qubit_matrix, _ = init_code.apply_random_logical()` (generate_data.py:131) on a batch:
    the operator draws of toric_model.py:234-248 / xzzx_model.py:346-355, applied by the device stencil."""
    from . import _surf, toric_model
    code = _CODES.get(code, code)
    n, size = m.shape[0], m.shape[-1]
    if code == L_.TORIC:
        for layer in range(2):
            ops = rng.integers(0, 4, size=n)
            xpos = np.where(np.isin(ops, (1, 2)), rng.integers(0, size, size=n), 0)
            zpos = np.where(np.isin(ops, (3, 2)), rng.integers(0, size, size=n), 0)
            m, _ = toric_model.apply_logical(m, ops, layer, xpos, zpos)
        return m
    ops = rng.integers(0, 4, size=n)
    xpos = np.where(np.isin(ops, (1, 2)), rng.integers(0, size, size=n), 0)
    zpos = np.where(np.isin(ops, (3, 2)), rng.integers(0, size, size=n), 0)
    if code == L_.PLANAR:
        from . import planar_model
        return planar_model.apply_logical(m, ops, xpos, zpos)[0]
    m, _ = _surf.apply_logical(code, m, ops, xpos, zpos)
    return m


def class_representatives(code, m):
    """uint8[n, ...] -> uint8[n, ncls, ...]: the configuration with the same syndrome in every equivalence class, indexed by
    class (`to_class(eq)` for the toric code, toric_model.py:354; for the 4-class codes the four logical operators, as
    STDC_Nall_n_alpha does with `apply_logical(eq_class ^ eq)`, decoders.py:557-561)."""
    from . import _surf, planar_model, toric_model
    code = _CODES.get(code, code)
    m = np.ascontiguousarray(m, dtype=np.uint8)
    if code == L_.TORIC:
        return np.stack([toric_model.to_class(m, eq) for eq in range(16)], axis=1)
    out = np.empty((m.shape[0], 4) + m.shape[1:], dtype=np.uint8)
    for op in range(4):
        r = planar_model.apply_logical(m, op)[0] if code == L_.PLANAR else _surf.apply_logical(code, m, op)[0]
        out[np.arange(m.shape[0]), np.asarray(_class_of(code, r))] = r
    return out


def rain(code, m, rng, p=0.5):
    """`apply_stabilizers_uniform` (toric_model.py:299-314, planar_model.py:355-376) on a batch: every generator is applied
    to every configuration independently with probability p (STDC's / STRC's high-energy start, decoders.py:246-247)."""
    from . import planar_model, toric_model
    code = _CODES.get(code, code)
    if code not in (L_.TORIC, L_.PLANAR):
        raise ValueError("rain is defined for the toric and planar codes (the only models with apply_stabilizers_uniform)")
    mod = toric_model if code == L_.TORIC else planar_model
    m = np.ascontiguousarray(m, dtype=np.uint8).copy()
    n, size = m.shape[0], m.shape[-1]
    pick = rng.random((n, 2, size, size)) < p
    if code == L_.PLANAR:                       # no X-type generator in the last row, no Z-type in the last column
        pick[:, 1, size - 1, :] = False
        pick[:, 0, :, size - 1] = False
    for o in range(2):
        for r in range(size):
            for c in range(size):
                sel = np.flatnonzero(pick[:, o, r, c])
                if sel.size:
                    m[sel] = mod.apply_stabilizer(m[sel], r, c, 3 if o == 0 else 1)[0]
    return m


def _estimate(method, code, reps, p_error, p_sampling, Nc, steps, droplets, conv_mult, seed, first, rng, alpha):
    """the unique-chain estimators of generate_data.py:168-196 on a batch of class representatives [n, ncls, ...] -> float[n, ncls]"""
    n = reps.shape[0]
    if method == "PTDC":                                                       # decoders.py:168-233
        hist = ptdc_batch(reps, p_sampling, Nc=Nc, steps=steps // Nc, droplets=droplets, conv_mult=conv_mult, seed=seed,
                          first_syndrome=first, code=code)
        return ptdc_distribution(hist, p_error)
    if method == "PTRC":                                                       # decoders.py:638-742
        n_u, m_o = ptdc_batch(reps, p_sampling, Nc=Nc, steps=steps // Nc, droplets=droplets, per_rung=True, with_m=True, seed=seed,
                              first_syndrome=first, code=code)
        return np.stack([ptrc_distribution(n_u[i], m_o[i], p_error, p_sampling) for i in range(n)]).astype(np.float64)
    if method in ("STDC", "STRC"):                                             # decoders.py:268-322, :835-949: rain per droplet
        starts = np.stack([rain(code, reps.reshape((-1,) + reps.shape[2:]), rng).reshape(reps.shape) for _ in range(droplets)], axis=2)
        if method == "STDC":
            hist = ptdc_batch(starts, p_sampling, Nc=1, steps=steps, droplets=droplets, iters=5, conv_mult=conv_mult, seed=seed,
                              first_syndrome=first, code=code)
            return ptdc_distribution(hist, p_error)
        n_u, m_o = ptdc_batch(starts, p_sampling, Nc=1, steps=steps, droplets=droplets, iters=5, with_m=True, conv_mult=conv_mult,
                              seed=seed, first_syndrome=first, code=code)
        return np.stack([strc_distribution(n_u[i], m_o[i], p_error, p_sampling) for i in range(n)])
    if method == "STDC_N_n":                                                   # decoders.py:537-581 (generate_data.py:190-196)
        _, xyz = ptdc_batch(reps, p_sampling, Nc=1, steps=steps, droplets=1, iters=5, with_xyz=True, alpha=alpha, seed=seed,
                            first_syndrome=first, code=code)
        return np.stack([nall_n_alpha_distribution(xyz[i], alpha, p_error) for i in range(n)])
    raise ValueError(f"method={method!r}")


def syndrome_of(code, m):
    """the defects of a batch of configurations in the flat layout qecmc_syndrome writes: uint8[n, cells]"""
    from . import _surf, planar_model, toric_model
    code = _CODES.get(code, code)
    m = np.ascontiguousarray(m, dtype=np.uint8)
    if code == L_.PLANAR:
        v, q = planar_model.syndrome(m)
        return np.concatenate([v.reshape(len(m), -1), q.reshape(len(m), -1)], axis=1).astype(np.uint8)
    d = toric_model.syndrome(m) if code == L_.TORIC else _surf.syndrome(code, m)
    return d.reshape(len(m), -1)


def _pteq_decode(params, init, seed, steps, conv_criteria, biased_decoder, metrics, pteq_kw):
    """generate's PTEQ call on a batch of start chains (generate_data.py:136-160) -> (pteq_batch's result, wall seconds, Nc)"""
    import time
    code, size, p = _CODES[params["code"]], params["size"], params["p_error"]
    noise = params.get("noise", "depolarizing")
    eta = params.get("eta") if noise == "biased" else None
    dec = dict(eta=eta)
    p_dec = p
    if noise == "alpha":
        dec = dict(alpha=params["alpha"])
    elif noise == "biased" and biased_decoder == "alpha":
        p_dec, a = biased_as_alpha(p, eta)
        dec = dict(alpha=float(a))
    Nc = params.get("Nc") or size
    t0 = time.perf_counter()
    if metrics not in ("basic", "full"):
        raise ValueError(f"metrics={metrics!r}")
    nq = int(np.prod(init.shape[1:]))
    swap_stats = metrics == "full" and Nc > 1 and int(pteq_kw.get("replicas", 1)) <= 1 and nq * int(steps) < 2 ** 32
    res = pteq_batch(init, p_dec, Nc=Nc, steps=steps, conv_criteria=conv_criteria, seed=seed, code=code, return_stats=True,
                     return_swap_stats=swap_stats, **dec, **pteq_kw)
    return res, time.perf_counter() - t0, Nc


def _exact_distr(params, chains, device):
    """params['method'] == "exact": the exact class law of every row (qecmc.exact_class_probabilities, DESIGN.md 4.1j .. 4.1m) under the weight of
    params['noise'] itself -- biased noise with the biased weight, whatever biased_decoder says; params['exact_method']: "auto" (default: coset
    enumeration where it takes the shape, the frontier sweep elsewhere, the cut-set sweep where both refuse), "enumerate", "sweep", "cut" or "tiled" (qecmc.exact) -- the sweep tiled
    over HBM only where it is named, with params['hbm_width'] and params['tile_width'] (0: the defaults).
    params['site_weights'] (an array as qecmc.class_sweep_site takes it: [..., 4] per cell, with or without a leading n) replaces the weight of
    params['noise'] by a weight per (row, qubit) -- erasures, a map of error rates, soft priors: the law is qecmc.exact_site_probabilities', with
    params['exact_method'] "auto" (default: the first of sweep, cut, tiled that takes the shape), "sweep", "cut" or "tiled" and the widths above."""
    from .exact import exact_class_probabilities, exact_site_probabilities
    if params.get("site_weights") is not None:
        if device != 0:
            raise ValueError("method exact under site weights runs on device 0: the library has no device-pointer form of it yet")
        return exact_site_probabilities(params["code"], chains, params["site_weights"], size=params["size"], method=params.get("exact_method", "auto"),
                                        lds_width=int(params.get("lds_width", 0)), hbm_width=int(params.get("hbm_width", 0)),
                                        tile_width=int(params.get("tile_width", 0)))
    noise = params.get("noise", "depolarizing")
    if _CODES[params["code"]] == L_.TORIC and noise != "depolarizing":
        raise ValueError(f"method exact on the toric code is defined for depolarizing noise, not {noise} (its errors are drawn without a bias)")
    kw = dict(eta=params["eta"]) if noise == "biased" else dict(alpha=params["alpha"]) if noise == "alpha" else {}
    if params.get("exact_method", "auto") == "tiled":
        kw.update(hbm_width=int(params.get("hbm_width", 0)), tile_width=int(params.get("tile_width", 0)))
    return exact_class_probabilities(params["code"], chains, params["p_error"], size=params["size"], chunk_bits=int(params.get("chunk_bits", 0)),
                                     device=device, method=params.get("exact_method", "auto"), **kw)


def _min_weight_distr(params, chains, device):
    """params['method'] == "min_weight": the class law carried by the shortest chains alone (qecmc.shortest_class_law) -- exact, by the
    (min, +, count) sweep: under depolarizing noise count * ((p / 3) / (1 - p))^(errors of the shortest chain), under the alpha model (an
    integer-valued params['alpha']) count * pz_tilde^(n_z + alpha n_xy).  Its argmax weighs a class's shortest chains by their number; as p -> 0 it is
    qecmc.min_weight_classes, the minimum-weight decoder.  params['lds_width'] (0: the default) as qecmc.class_minplus takes it.  Biased noise is
    refused: its weights are no integer powers of one base.  params['exact_method'] = "tiled" runs the sweep tiled over HBM instead
    (qecmc.class_minplus_tiled, DESIGN.md 4.1r: rotated L = 13 .. 21, planar L = 8 .. 12, toric L = 7) with params['hbm_width'] and
    params['tile_width'] (0: the defaults), as _exact_distr takes them; it runs only where it is named.
    params['site_costs'] (a table as qecmc.class_minplus_site takes it: integer [..., 4] per cell, with or without a leading n) replaces the four
    costs of params['noise'] by a cost per (row, qubit) -- erasures, any costs that are exponents of the noise's base: the law is
    count * base^cost under the table, base formed from p_error / alpha as above."""
    from .exact import shortest_class_law
    noise = params.get("noise", "depolarizing")
    if noise == "biased":
        raise ValueError("method min_weight is defined for depolarizing and alpha noise, not biased: the biased weights are no integer powers of one base")
    if _CODES[params["code"]] == L_.TORIC and noise != "depolarizing":
        raise ValueError(f"method min_weight on the toric code is defined for depolarizing noise, not {noise} (its errors are drawn without a bias)")
    if device != 0:
        raise ValueError("method min_weight runs on device 0: the library has no device-pointer form of it yet")
    kw = dict(lds_width=int(params.get("lds_width", 0)))
    if params.get("exact_method") == "tiled":                                   # (only where it is named: every other value leaves the cut plans, as before)
        kw = dict(method="tiled", hbm_width=int(params.get("hbm_width", 0)), tile_width=int(params.get("tile_width", 0)))
    return shortest_class_law(params["code"], chains, params["p_error"], alpha=params["alpha"] if noise == "alpha" else None, size=params["size"],
                              site_costs=params.get("site_costs"), **kw)


def _corrections_for(code, size, candidates, distr, device):
    """the correction of every row towards target = argmax(distr) -- the very expression `success` uses -- from candidates [n, K, ...] or [n, ...]"""
    from .syndrome_corrections import corrections as correct
    target = np.argmax(distr, axis=1).astype(np.int32)
    return target, correct(code, candidates, target, device=device, size=size)


def _correction_route(params, method):
    """params['correction']: None (default: qecmc.corrections -- class move and greedy descent), "shortest" (method min_weight on the cut plans: the
    traced shortest chain of the target class, qecmc.shortest_chains) or "shortest_tiled" (method min_weight with
    params['exact_method'] = "tiled": qecmc.shortest_chains_tiled); refused by name under any other method or route"""
    route = params.get("correction")
    if route not in (None, "shortest", "shortest_tiled"):
        raise ValueError(f"params['correction']={route!r}: 'shortest', 'shortest_tiled', or absent for qecmc.corrections")
    if route is not None and method != "min_weight":
        raise ValueError(f"params['correction']={route!r} is built for method min_weight, not {method}: only the (min, +) sweep traces a shortest chain")
    if route == "shortest" and params.get("exact_method") == "tiled":
        raise ValueError("params['correction']='shortest' is not built for params['exact_method']='tiled': the tiled (min, +) sweep has no traceback; "
                         "leave 'correction' out for qecmc.corrections (its own traceback goes by params['correction']='shortest_tiled')")
    if route == "shortest_tiled" and params.get("exact_method") != "tiled":
        raise ValueError(f"params['correction']='shortest_tiled' is built for params['exact_method']='tiled', not {params.get('exact_method')!r}: "
                         "the cut plans trace by params['correction']='shortest'")
    return route


def _site_costs_route(params, method):
    """params['site_costs'] (qecmc.class_minplus_site's table) is built for method min_weight; refused by name under any other method"""
    if params.get("site_costs") is not None and method != "min_weight":
        raise ValueError(f"params['site_costs'] is built for method min_weight, not {method}: method exact takes params['site_weights']")


def _shortest_corrections_for(params, chains, distr, device):
    """_corrections_for by params['correction'] = "shortest" / "shortest_tiled": target = argmax(distr) and, in the keys of qecmc.corrections, the traced shortest chain of
    that class under the costs _min_weight_distr decodes with -- params['site_costs'] where given -- weight its error count, source 0, moved: target is
    not the start chain's class"""
    from .exact import shortest_chains, shortest_chains_site, shortest_chains_tiled, shortest_chains_tiled_site
    noise = params.get("noise", "depolarizing")
    if device != 0:
        raise ValueError("method min_weight runs on device 0: the library has no device-pointer form of it yet")
    costs = (0, int(params["alpha"]), int(params["alpha"]), 1) if noise == "alpha" else (0, 1, 1, 1)
    target = np.argmax(distr, axis=1).astype(np.int32)
    if params.get("correction") == "shortest_tiled":                            # (the widths _min_weight_distr swept with)
        kw = dict(size=params["size"], hbm_width=int(params.get("hbm_width", 0)), tile_width=int(params.get("tile_width", 0)))
        one, site = shortest_chains_tiled, shortest_chains_tiled_site
    else:
        kw = dict(size=params["size"], lds_width=int(params.get("lds_width", 0)))
        one, site = shortest_chains, shortest_chains_site
    if params.get("site_costs") is not None:
        r = site(params["code"], chains, params["site_costs"], **kw)
    else:
        r = one(params["code"], chains, costs, **kw)
    cor = r["chains"][np.arange(len(target)), target]
    return target, dict(corrections=cor, weight=(cor != 0).reshape(len(cor), -1).sum(axis=1).astype(np.int32), source=np.zeros(len(cor), np.int32),
                        moved=(target != r["cls"]).astype(np.uint8))


def _correction_outputs(code, size, raw, init, distr, device, params=None):
    """generate's corrections=True: the correction of every start chain towards argmax(distr), its weight, and whether raw ^ correction is a stabilizer"""
    if params is not None and params.get("correction") in ("shortest", "shortest_tiled"):
        _, cor = _shortest_corrections_for(params, init, distr, device)
    else:
        _, cor = _corrections_for(code, size, init, distr, device)
    residual = raw ^ cor["corrections"]
    stabilizer_class = int(np.asarray(_class_of(code, np.zeros_like(raw[:1])))[0])
    return dict(correction=cor["corrections"], correction_weight=cor["weight"],
                success_correction=~syndrome_of(code, residual).any(axis=1) & (np.asarray(_class_of(code, residual)) == stabilizer_class))


def decode_syndromes(params, defects, seed=0, steps=100000, conv_criteria="error_based", biased_decoder="alpha", metrics="basic", corrections=False,
                     correction_candidates="lift", **pteq_kw):
    """Decode BARE SYNDROMES: `defects` (as qecmc.chains_from_syndromes takes them, for params['code'] / params['size']) are lifted to start
    chains on the device and decoded exactly as `generate` decodes its seed configurations for params['method'] == "PTEQ" -- the same
    decoder routing by params['noise'], the same keywords.  The start chain is a local minimum of the weight in an arbitrary class: the
    class law does not depend on it, only the burn-in does.
    Returns dict(distr, counts, steps_done, converged, samples, tops0, chains, status, weight); raises if a syndrome is none of the code.
    params['method'] = "exact" decodes by coset enumeration instead (qecmc.exact_class_probabilities under the weight of params['noise'] itself;
    params['chunk_bits'] optional): distr float64[n, ncls], chains, status, weight -- no counts, no run.  params['site_weights'] is passed through:
    the exact law under a weight per (row, qubit) (_exact_distr).  params['method'] = "min_weight" returns the same keys with distr the law of the
    shortest chains alone (_min_weight_distr); params['site_costs'] (method min_weight only, refused by name elsewhere) decodes under a cost per
    (row, qubit), and params['correction'] = "shortest" then traces under the same table.
    corrections=True adds what a user who measured a syndrome wants (qecmc.corrections): target = argmax(distr) per row, correction -- a
    chain with the syndrome in that class --, correction_weight, correction_source and correction_moved.  The candidate is the lifted chain;
    correction_candidates="states" adds the Nc final rung states of every ladder as candidates 1 ..., where the route returns them: a fixed-length
    run (conv_criteria=None).  A run the convergence criterion stops may go to the work-queue kernels, which write no final states: ValueError.
    params['correction'] = "shortest" (method min_weight only, refused by name elsewhere): correction is the traced shortest chain of the target class
    (qecmc.shortest_chains) instead of qecmc.corrections' class move and descent; correction_source is 0 and correction_moved says whether the target
    is another class than the lifted chain's.  params['correction'] = "shortest_tiled" is the same on the tiled route (params['exact_method'] = "tiled",
    qecmc.shortest_chains_tiled), refused by name elsewhere."""
    from .syndrome_lift import chains_from_syndromes
    method = params.get("method", "PTEQ")
    if method not in ("PTEQ", "exact", "min_weight"):
        raise ValueError("decode_syndromes decodes with PTEQ, exact or min_weight (params['method'])")
    route = _correction_route(params, method)
    _site_costs_route(params, method)
    noise = params.get("noise", "depolarizing")
    if noise not in ("depolarizing", "biased", "alpha"):
        raise ValueError(f"noise={noise!r}")
    lifted = chains_from_syndromes(params["code"], defects, device=int(pteq_kw.get("device", 0)), size=params["size"])
    chains, status, weight = lifted["chains"], np.atleast_1d(lifted["status"]), np.atleast_1d(lifted["weight"])
    if chains.ndim == (3 if _CODES[params["code"]] in (L_.TORIC, L_.PLANAR) else 2):
        chains = chains[None]
    if status.any():
        raise ValueError("not syndromes of the %s code: rows %s" % (params["code"], np.flatnonzero(status)[:8].tolist()))
    if correction_candidates not in ("lift", "states"):
        raise ValueError(f"correction_candidates={correction_candidates!r}")
    with_states = bool(corrections) and correction_candidates == "states"
    if method in ("exact", "min_weight"):
        if with_states:
            raise ValueError(f"correction_candidates='states': method {method} runs no ladder; keep the lifted chain")
        distr_of = _exact_distr if method == "exact" else _min_weight_distr
        out = dict(distr=distr_of(params, chains, int(pteq_kw.get("device", 0))), chains=chains, status=status, weight=weight)
        if corrections:
            if route in ("shortest", "shortest_tiled"):
                target, cor = _shortest_corrections_for(params, chains, out["distr"], int(pteq_kw.get("device", 0)))
            else:
                target, cor = _corrections_for(_CODES[params["code"]], params["size"], chains, out["distr"], int(pteq_kw.get("device", 0)))
            out.update(target=target, correction=cor["corrections"], correction_weight=cor["weight"], correction_source=cor["source"],
                       correction_moved=cor["moved"])
        return out
    if with_states:
        if conv_criteria is not None:
            raise ValueError(f"correction_candidates='states': the route conv_criteria={conv_criteria!r} (a run stopped by the convergence criterion, which may "
                             "take the work-queue kernels) returns no final states; decode with conv_criteria=None or keep the lifted chain")
        pteq_kw = dict(pteq_kw, return_states=True)
    res, _, _ = _pteq_decode(params, chains, seed, steps, conv_criteria, biased_decoder, metrics, pteq_kw)
    out = dict(distr=res["percent"], counts=res["counts"], steps_done=res["steps_done"], converged=res["converged"], samples=res["samples"],
               tops0=res["tops0"], chains=chains, status=status, weight=weight)
    if corrections:
        cand = chains
        if with_states:                                            # [n * replicas, Nc, ...] -> the lifted chain, then every final rung state of the row
            n = chains.shape[0]
            cand = np.concatenate([chains[:, None], res["states"].reshape((n, -1) + chains.shape[1:])], axis=1)
        target, cor = _corrections_for(_CODES[params["code"]], params["size"], cand, out["distr"], int(pteq_kw.get("device", 0)))
        out.update(target=target, correction=cor["corrections"], correction_weight=cor["weight"], correction_source=cor["source"],
                   correction_moved=cor["moved"])
    return out


def _qubit_cells(code, size):
    """bool[...]: the cells of the state layout that hold a qubit -- all of them, but for the planar code's layer 1, which lives on its first
    size - 1 rows and columns (planar_model.py:38-39)"""
    code = _CODES.get(code, code)
    cells = np.ones((2, size, size) if code in (L_.TORIC, L_.PLANAR) else (size, size), dtype=bool)
    if code == L_.PLANAR:
        cells[1, -1, :] = False
        cells[1, :, -1] = False
    return cells


def draw_erasures(code, size, n, p_erase, rng):
    """bool[n, ...]: every qubit of every shot erased independently with probability p_erase; the planar code's unused cells are never erased"""
    cells = _qubit_cells(code, size)
    return (rng.random((n,) + cells.shape) < p_erase) & cells


def apply_erasures(m, erased, rng):
    """the error chains m uint8[n, ...] with a uniform one of I, X, Y, Z put on every erased cell (whatever was there: an erased qubit is lost)"""
    m = np.array(m, dtype=np.uint8)
    erased = np.asarray(erased, dtype=bool)
    m[erased] = rng.integers(0, 4, size=int(erased.sum()), dtype=np.uint8)
    return m


def erasure_experiment(params, n, seed=0, method="exact"):
    """n shots of params['code'] at params['size'] under the noise of params (p_error, noise, eta as draw_errors takes them) AND erasures: every qubit
    erased with probability params['p_erase'], an erased qubit carrying a uniform Pauli.  Decoded from the BARE syndromes by the maximum-likelihood
    decoder that knows each shot's erased set: decode_syndromes, method exact, under qecmc.erasure_site_w4 of the noise's weights
    (params['exact_method'] and the widths as _exact_distr takes them; p_error = 0 is the pure-erasure channel, weights (1, 0, 0, 0) off the set).
    method="min_weight" decodes the same shots -- the same draws for the same seed -- by the shortest chains instead (decode_syndromes, method
    min_weight) under qecmc.erasure_site_costs of the noise's costs: (0, 1, 1, 1) for depolarizing noise, (0, alpha, alpha, 1) for
    the alpha model with an integer alpha, an erased qubit free; biased noise is refused as _min_weight_distr refuses it.
    Returns dict(distr float64[n, ncls], eq_true: the class of the true error, success: argmax(distr) == eq_true, erased bool[n, ...], chains: the
    start chains the syndromes were lifted to).  params['correction'] ("shortest", or "shortest_tiled" with params['exact_method'] = "tiled"; method
    min_weight) adds target, correction -- the shortest chain of the target class under the shot's erasure costs -- and correction_weight, its error
    count (erased cells included)."""
    from .exact import alpha_w4, biased_w4, depolarizing_w4, erasure_site_costs, erasure_site_w4
    code, size, p = _CODES[params["code"]], params["size"], params["p_error"]
    noise = params.get("noise", "depolarizing")
    if noise not in ("depolarizing", "biased", "alpha"):
        raise ValueError(f"noise={noise!r}")
    if method not in ("exact", "min_weight"):
        raise ValueError(f"method={method!r}: erasure_experiment decodes with 'exact' or 'min_weight'")
    if method == "min_weight":
        if noise == "biased":
            raise ValueError("method min_weight is defined for depolarizing and alpha noise, not biased: the biased weights are no integer powers of one base")
        if noise == "alpha" and (float(params["alpha"]) != np.floor(float(params["alpha"])) or not 0 <= float(params["alpha"]) <= 255):
            raise ValueError(f"alpha={params['alpha']!r}: method min_weight takes integer costs, so an integer-valued alpha in 0 .. 255")
    rng = np.random.default_rng(seed)
    if noise == "alpha":
        errors = draw_errors(code, size, n, p, rng, rates=alpha_rates(p, params["alpha"]))
        base = alpha_w4(p, params["alpha"])
    else:
        eta = params.get("eta") if noise == "biased" and code != L_.TORIC else None
        errors = draw_errors(code, size, n, p, rng, eta=eta)
        base = depolarizing_w4(p) if eta is None else biased_w4(p, eta)
    erased = draw_erasures(code, size, n, params["p_erase"], rng)
    errors = apply_erasures(errors, erased, rng)
    if method == "min_weight":
        costs = (0, int(params["alpha"]), int(params["alpha"]), 1) if noise == "alpha" else (0, 1, 1, 1)
        decode = dict(params, method="min_weight", site_costs=erasure_site_costs(costs, erased))
        decode.pop("site_weights", None)
    else:
        decode = dict(params, method="exact", site_weights=erasure_site_w4(base, erased))
    traced = decode.get("correction") is not None                               # (method min_weight only: _correction_route refuses it elsewhere)
    out = decode_syndromes(decode, syndrome_of(code, errors), corrections=traced)
    eq_true = np.asarray(_class_of(code, errors)).astype(np.int32)
    res = dict(distr=out["distr"], eq_true=eq_true, success=np.argmax(out["distr"], axis=1) == eq_true, erased=erased, chains=out["chains"])
    if traced:
        res.update(target=out["target"], correction=out["correction"], correction_weight=out["correction_weight"])
    return res


def generate(params, nbr_datapoints, seed=0, file_path=None, steps=100000, conv_criteria="error_based", biased_decoder="alpha",
             rng=None, device_generation=False, metrics="basic", start="error", corrections=False, **pteq_kw):
    """params: dict like generate_data.py:276-296 ({'code','size','p_error','noise'[,'eta','alpha']}), method PTEQ.
    noise 'depolarizing' -> PTEQ (:136); 'biased' -> errors from the eta split (:78-83) decoded by PTEQ_alpha with
    (pz_tilde, alpha) derived from (p, eta) exactly as :142-150 does (biased_decoder="biased" decodes with PTEQ_biased
    instead); 'alpha' -> p_error is pz_tilde, errors and decoder from (pz_tilde, alpha) (:84-91,:151-160).
    params['method'] = "PTEQ_with_shortest" (alpha noise, generate_data.py:167-173) runs pteq_shortest_batch (scan "wave" unless given) and keeps the three
    vectors of PTEQ_alpha_with_shortest per datapoint: distr, distr_shortest, distr_shortest_n (success from the first).
    params['method'] (default "PTEQ") may also be "PTDC", "PTRC", "STDC", "STRC" or "STDC_N_n" (generate_data.py:168-196): the
    unique-chain estimators on one representative per class of every syndrome, with params['p_sampling'] (default p_error),
    params['droplets'], params['conv_mult'] and `steps` as the estimator's own `steps`; `batch` syndromes go into one launch
    (default 256: the sets of visited chains live in HBM).  They return distr float64[n, ncls] and no counts.
    params['method'] = "exact" is the maximum-likelihood decoder of the small codes: distr float64[n, ncls] is the exact class law of every
    syndrome by coset enumeration on the device (qecmc.exact_class_probabilities) under the weight of params['noise'] itself --
    biased noise with the biased weight, whatever biased_decoder says --, with success and no counts; start="syndrome" and corrections=True work
    on top of it; `steps` and the sampler keywords are not looked at.
    params['method'] = "min_weight" decodes by the shortest chains: distr float64[n, ncls] is the law carried by the shortest chains of every class
    alone, exact (qecmc.shortest_class_law; depolarizing noise, or alpha noise with an integer alpha; biased noise is refused), with
    success and no counts; start="syndrome" and corrections=True work as they do for "exact".  params['site_costs'] (method min_weight only, refused by
    name under any other) decodes under a cost per (row, qubit) (qecmc.class_minplus_site), and params['correction'] = "shortest"
    traces under the same table.
    device_generation=True draws the errors and the hiding logical operator on the GPU (`generate_syndromes`) instead of NumPy.
    start="error" (default) is the reference's recipe: the decoder starts from the error with a random logical operator on top.  start="syndrome"
    (methods PTEQ, exact and min_weight) lets nothing but syndrome(raw) reach the decoder: the start chains are qecmc.chains_from_syndromes of it and no logical
    operator is drawn; eq_true and the success rule are the same.
    metrics="basic" (default) costs nothing: throughput, convergence, burn-in and success figures.  metrics="full" also attaches the
    mixing counters (swap acceptance per rung pair, mean error count per rung) -- which rule out the work-queue kernels
    (their lanes run several ladders) and need nq * steps < 2^32, so they are dropped, not failed on, where they do not fit.
    corrections=True (methods PTEQ, exact and min_weight) closes the loop: correction uint8[n,...] is qecmc.corrections of the start chain -- the seed configuration, or the
    lifted chain of start="syndrome" -- towards argmax(distr), correction_weight its error count, and success_correction[s] is true iff
    raw[s] ^ correction[s] (byte values XOR as the Pauli product) is a stabilizer: an all-zero syndrome and the class of the zero chain.
    params['correction'] = "shortest" (method min_weight with corrections=True; refused by name under any other method) makes correction the traced
    shortest chain of argmax(distr) instead (qecmc.shortest_chains): no chain of that class is lighter; correction_weight and
    success_correction keep their meaning.  The default stays the qecmc.corrections route.  params['correction'] = "shortest_tiled" is the same with
    params['exact_method'] = "tiled" (qecmc.shortest_chains_tiled, DESIGN.md 4.1u: rotated L = 13 .. 21, planar L = 8 .. 12, toric L = 7), refused by name elsewhere;
    "shortest" stays refused there.
    Returns (and optionally saves as npz) qubit_matrix uint8[n,...] (the raw errors, generate_data.py:120),
    eq_true int32[n], counts uint32[n,ncls], distr uint8[n,ncls] (what PTEQ returns), success bool[n]
    (argmax(distr) == eq_true, generate_data.py:139), steps_done, converged."""
    code = _CODES[params["code"]]
    size, p = params["size"], params["p_error"]
    noise = params.get("noise", "depolarizing")
    if noise not in ("depolarizing", "biased", "alpha"):
        raise ValueError(f"noise={noise!r}")
    eta = params.get("eta") if noise == "biased" else None
    rng = np.random.default_rng(seed) if rng is None else rng         # (shards pass a generator keyed by (seed, shard id))
    rates = alpha_rates(p, params["alpha"]) if noise == "alpha" else None
    method = params.get("method", "PTEQ")
    if start not in ("error", "syndrome"):
        raise ValueError(f"start={start!r}")
    if start == "syndrome" and method not in ("PTEQ", "exact", "min_weight"):
        raise ValueError(f"start='syndrome' is built for methods PTEQ, exact and min_weight, not {method}")
    if corrections and method not in ("PTEQ", "exact", "min_weight"):
        raise ValueError(f"corrections=True is built for methods PTEQ, exact and min_weight, not {method}")
    if method == "min_weight" and noise == "biased":
        raise ValueError("method min_weight is defined for depolarizing and alpha noise, not biased: the biased weights are no integer powers of one base")
    _correction_route(params, method)
    _site_costs_route(params, method)
    if device_generation:
        # errors, true class and the hiding logical operator drawn on the GPU (Philox keyed by the global syndrome index: the data
        # set does not depend on how it is cut into shards)
        init, raw, eq_true = generate_syndromes(code, size, nbr_datapoints, p, eta, rates, start == "error", seed, int(pteq_kw.get("first_syndrome", 0)))
    else:
        raw = draw_errors(code, size, nbr_datapoints, p, rng, eta, rates=rates)
        eq_true = np.asarray(_class_of(code, raw), dtype=np.int32)
        init = hide_class(code, raw, rng) if start == "error" else raw
    if start == "syndrome":
        from .syndrome_lift import chains_from_syndromes
        init = chains_from_syndromes(code, syndrome_of(code, raw), device=int(pteq_kw.get("device", 0)), size=size)["chains"]
    if method == "PTEQ_with_shortest":                                         # generate_data.py:167-173, PTEQ_alpha_with_shortest on the whole batch
        if noise != "alpha":
            raise ValueError("method PTEQ_with_shortest is defined for alpha noise (generate_data.py:167-173)")
        from .decoders_biasednoise import pteq_shortest_batch, shortest_distribution
        pteq_kw.setdefault("scan", "wave")
        res = pteq_shortest_batch(init, p, params["alpha"], Nc=params.get("Nc") or size, steps=steps, conv_criteria=conv_criteria, seed=seed, code=code,
                                  **pteq_kw)
        distr, distr_shortest, distr_shortest_n = shortest_distribution(res, p)
        out = dict(qubit_matrix=raw, eq_true=eq_true, counts=res["counts"], distr=distr, distr_shortest=distr_shortest, distr_shortest_n=distr_shortest_n,
                   success=np.argmax(distr, axis=1) == eq_true, steps_done=res["steps_done"], converged=res["converged"], samples=res["samples"],
                   tops0=res["tops0"], overflow=res["overflow"])
        if file_path is not None:
            np.savez_compressed(file_path, params=np.array([repr(params)]), **out)
        return out
    if method in ("exact", "min_weight"):
        distr = (_exact_distr if method == "exact" else _min_weight_distr)(params, init, int(pteq_kw.get("device", 0)))
        out = dict(qubit_matrix=raw, eq_true=eq_true, distr=distr, success=np.argmax(distr, axis=1) == eq_true)
        if corrections:
            out.update(_correction_outputs(code, size, raw, init, distr, int(pteq_kw.get("device", 0)), params))
        if file_path is not None:
            np.savez_compressed(file_path, params=np.array([repr(params)]), **out)
        return out
    if method != "PTEQ":
        if noise != ("alpha" if method == "STDC_N_n" else "depolarizing"):
            raise ValueError(f"method {method} is defined for {'alpha' if method == 'STDC_N_n' else 'depolarizing'} noise (generate_data.py:168-196)")
        batch = int(pteq_kw.pop("batch", 256))
        ncls = 16 if code == L_.TORIC else 4
        distr = np.empty((nbr_datapoints, ncls), dtype=np.float64)
        droplets = params.get("droplets", 1 if method == "STDC_N_n" else 4)
        for lo in range(0, nbr_datapoints, batch):
            reps = class_representatives(code, init[lo:lo + batch])
            # every (syndrome, class, droplet) ladder needs a Philox syndrome index of its own
            distr[lo:lo + batch] = _estimate(method, code, reps, p, params.get("p_sampling") or p, params.get("Nc") or size, steps, droplets,
                                             params.get("conv_mult", 0), seed, lo * ncls * droplets, rng, params.get("alpha"))
        out = dict(qubit_matrix=raw, eq_true=eq_true, distr=distr, success=np.argmax(distr, axis=1) == eq_true)
        if file_path is not None:
            np.savez_compressed(file_path, params=np.array([repr(params)]), **out)
        return out
    res, wall, Nc = _pteq_decode(params, init, seed, steps, conv_criteria, biased_decoder, metrics, pteq_kw)
    out = dict(qubit_matrix=raw, eq_true=eq_true, counts=res["counts"], distr=res["percent"],
               success=np.argmax(res["percent"], axis=1) == eq_true, steps_done=res["steps_done"],
               converged=res["converged"], samples=res["samples"], tops0=res["tops0"])
    if corrections:
        out.update(_correction_outputs(code, size, raw, init, out["distr"], int(pteq_kw.get("device", 0))))
    if file_path is not None:
        np.savez_compressed(file_path, params=np.array([repr(params)]), **out)
    out["metrics"] = batch_metrics(code, size, Nc, int(pteq_kw.get("iters", 10)), res, wall, out["success"],
                                   replicas=int(pteq_kw.get("replicas", 1)), scan=pteq_kw.get("scan", "random"),
                                   first_syndrome=int(pteq_kw.get("first_syndrome", 0)))
    return out


def wavefront_clusters(n, replicas=1, first_syndrome=0):
    """scan = "wave" shares the generator picks of the 64 ladders whose global indices lie in one group of 64 (ladder l of
    syndrome s: first_syndrome + s * replicas + r), so the results of the syndromes with ladders in one group are correlated.
    Returns int64[n]: a cluster id per syndrome -- syndromes that share a group, directly or through a neighbour, share an id."""
    R = max(int(replicas), 1)
    start = int(first_syndrome) + np.arange(int(n), dtype=np.int64) * R
    g0, g1 = start // 64, (start + R - 1) // 64
    new = np.ones(int(n), dtype=bool)
    new[1:] = g0[1:] > g1[:-1]
    return np.cumsum(new) - 1


def _is_wave(scan):
    return scan in ("wave", L_.SCAN_WAVE)


def success_err(success, scan="random", replicas=1, first_syndrome=0, clusters=None):
    """Standard error of the success rate -> (err, binomial err, method).  scan = "wave": over the clusters of syndromes that share
    picks (wavefront_clusters; the ratio estimator's cluster variance K/(K-1) sum_k (y_k - p n_k)^2 / n^2, which is the standard
    error of the cluster means when the clusters are equal), nan for a single cluster; other scans: the binomial error."""
    s = np.asarray(success, dtype=np.float64)
    n = len(s)
    k = float(s.mean()) if n else float("nan")
    binom = float(np.sqrt(max(k * (1 - k), 0.0) / n)) if n else float("nan")
    if not _is_wave(scan):
        return binom, binom, "binomial"
    cl = wavefront_clusters(n, replicas, first_syndrome) if clusters is None else np.asarray(clusters)
    _, cl = np.unique(cl, return_inverse=True)
    K = int(cl.max()) + 1 if n else 0
    if K < 2:
        return float("nan"), binom, "wavefront_clusters"
    y, m = np.bincount(cl, weights=s, minlength=K), np.bincount(cl, minlength=K).astype(np.float64)
    return float(np.sqrt(K / (K - 1.0) * np.sum((y - k * m) ** 2)) / n), binom, "wavefront_clusters"


def batch_metrics(code, size, Nc, iters, res, wall_s, success=None, replicas=1, scan="random", first_syndrome=0):
    """The per-batch metrics line (SURVEY.md 5 "Metrics / logging"; the reference only prints a progress counter,
    generate_data.py:266): proposals, seconds, chain-sweeps/s, swap acceptance per rung pair, mean error count per rung,
    the tops0 histogram, and the success rate when the true classes are known.  JSON-serialisable.
    success_rate_err is the binomial error, except on scan = "wave", where the syndromes of a wavefront share their generator
    picks and the error is taken over the clusters of syndromes that share them (success_err); success_rate_err_method says which,
    success_rate_err_binomial keeps the binomial value."""
    n_gen = 2 * size * size if code == L_.TORIC else 2 * size * (size - 1) if code == L_.PLANAR else size * size - 1
    steps_run = res["steps_done"].astype(np.float64)
    proposals = float(steps_run.sum()) * Nc * iters * max(int(replicas), 1)
    k_ms = res.get("stats", {}).get("kernel_ms", float("nan"))
    m = dict(syndromes=int(res["counts"].shape[0]), Nc=int(Nc), iters=int(iters), proposals=proposals, wall_s=float(wall_s),
             kernel_ms=float(k_ms), chain_sweeps_per_s_kernel=float(proposals / n_gen / (k_ms * 1e-3)) if k_ms == k_ms and k_ms > 0 else None,
             chain_sweeps_per_s_wall=float(proposals / n_gen / wall_s) if wall_s > 0 else None,
             converged_frac=float(np.mean(res["converged"])), mean_steps=float(steps_run.mean()) if steps_run.size else 0.0,
             frac_past_burn_in=float(np.mean(res["samples"] > 0)) if res["samples"].size else 0.0,
             tops0_hist=np.bincount(np.minimum(res["tops0"], 20).astype(np.int64), minlength=21).tolist())
    if "swap_accepts" in res and steps_run.sum() > 0:
        m["swap_acceptance"] = (res["swap_accepts"].sum(axis=0) / steps_run.sum()).tolist()
        m["mean_errors_per_rung"] = (res["nerr_sums"].sum(axis=0) / steps_run.sum()).tolist()
    if success is not None and len(success):
        k, n = int(np.sum(success)), len(success)
        m["success_rate"] = k / n
        err, binom, how = success_err(success, scan, replicas, first_syndrome)
        m["success_rate_err"], m["success_rate_err_binomial"], m["success_rate_err_method"] = err, binom, how
    return m


def shard_name(prefix, seed, shard):
    return f"{prefix}_seed{int(seed)}_shard{int(shard):05d}.npz"


def generate_shards(params, n_total, shard_size, out_dir, seed=0, prefix="data", log=None, **gen_kw):
    """The reference's array job (generate_data.py:251-256,274-276; generate_data_noise_models.py:27-32): the data set is cut
    into shards keyed by (seed, shard id); a shard whose file exists is skipped, so an interrupted job resumes where it
    stopped, and any subset of shards can be (re)made on any GPU in any order with the same result -- shard k draws its
    errors from default_rng([seed, k]) and its ladders from Philox syndrome indices k*shard_size ....
    One JSON metrics line per shard made is appended to <out_dir>/<prefix>_metrics.jsonl (and to `log`, a list, if given).
    Returns the list of shard paths (all of them, made or found)."""
    import json
    import os
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    n_shards = (int(n_total) + int(shard_size) - 1) // int(shard_size)
    for k in range(n_shards):
        path = os.path.join(out_dir, shard_name(prefix, seed, k))
        paths.append(path)
        if os.path.exists(path):                                   # resume = skip existing shards
            continue
        n = min(int(shard_size), int(n_total) - k * int(shard_size))
        tmp = path + ".tmp.npz"
        out = generate(params, n, seed=seed, file_path=tmp, rng=np.random.default_rng([int(seed), k]),
                       first_syndrome=k * int(shard_size) * max(int(gen_kw.get("replicas", 1)), 1), **gen_kw)
        os.replace(tmp, path)                                      # a shard file is complete or absent
        line = dict(shard=k, seed=int(seed), file=os.path.basename(path), **out.get("metrics", {}))
        with open(os.path.join(out_dir, f"{prefix}_metrics.jsonl"), "a") as f:
            f.write(json.dumps(line) + "\n")
        if log is not None:
            log.append(line)
    return paths


def threshold_curve(params, p_list, n, seed=0, **gen_kw):
    """Logical success rate against the physical error rate (the p_error scan of generate_data.py:57-60,121-141,276-296 --
    the reference loops p over [0.05, 0.20] in its job script and evaluates argmax(distr) == true class offline):
    for every p in p_list, n syndromes at p_error = p decoded in one batched call.
    Returns dict(p, n, success_rate, err (standard error), converged_frac, metrics [one dict per p]) and, beside the raw
    rate, success_rate_sampled / err_sampled / frac_sampled: the rate among the syndromes whose ladder got past the burn-in
    (samples > 0).  The reference's burn-in trap (decoders.py:63,89: a ladder that never sees tops0 >= tops_burn returns an all-zero
    vector, argmax 0) counts as a failure in the raw rate; at low p and a short horizon it, not the decoder, sets that number.
    err / err_sampled are binomial except on scan = "wave" (errors over the clusters of syndromes that share generator picks,
    success_err); err_binomial / err_sampled_binomial keep the binomial values and err_method says which is reported."""
    rate, err, conv, met, rate_s, err_s, frac_s, err_b, err_sb = [], [], [], [], [], [], [], [], []
    scan, R, first = gen_kw.get("scan", "random"), int(gen_kw.get("replicas", 1)), int(gen_kw.get("first_syndrome", 0))
    how = "binomial"
    for i, p in enumerate(p_list):
        out = generate(dict(params, p_error=float(p)), n, seed=seed + i, **gen_kw)
        k = float(np.mean(out["success"]))
        e, eb, how = success_err(out["success"], scan, R, first)
        rate.append(k); err.append(e); err_b.append(eb)
        conv.append(float(np.mean(out["converged"])) if "converged" in out else float("nan"))
        met.append(out.get("metrics"))
        sampled = out["samples"] > 0 if "samples" in out else np.ones(len(out["success"]), dtype=bool)
        ns = int(sampled.sum())
        ks = float(np.mean(out["success"][sampled])) if ns else float("nan")
        es, esb, _ = success_err(out["success"][sampled], scan, clusters=wavefront_clusters(len(sampled), R, first)[sampled]) if ns \
            else (float("nan"),) * 3
        rate_s.append(ks); err_s.append(es); err_sb.append(esb); frac_s.append(ns / max(n, 1))
    return dict(p=np.asarray(p_list, dtype=np.float64), n=int(n), success_rate=np.array(rate), err=np.array(err),
                converged_frac=np.array(conv), metrics=met, success_rate_sampled=np.array(rate_s), err_sampled=np.array(err_s),
                frac_sampled=np.array(frac_s), err_binomial=np.array(err_b), err_sampled_binomial=np.array(err_sb), err_method=how)


def grown_log_rows(log_rows, steps_done, steps, growth=2):
    """The log of a criterion `LadderRun` before a chunk of `steps` ladder steps behind `steps_done`: (rows it must have, rows to carry over).
    Rows are absolute ladder steps, so the log grows by appending rows: geometrically (x `growth`), at least to steps_done + steps; the
    steps_done rows written so far are copied into the new buffer.  (log_rows, 0): it is large enough as it is."""
    log_rows, steps_done, steps = int(log_rows), int(steps_done), int(steps)
    need = steps_done + steps
    if need <= log_rows:
        return log_rows, 0
    return max(need, int(growth) * log_rows), min(steps_done, log_rows)


def packed_neff(states):
    """uint8[..., nq] Pauli configurations -> uint32[...]: n_z | (n_x + n_y) << 16, the form the alpha-noise ladders carry their
    n_eff attributes in (Chain_alpha.__init__, mcmc_alpha.py:18-22)"""
    a = np.asarray(states)
    return ((a == 3).sum(axis=-1).astype(np.uint32) | (((a == 1) | (a == 2)).sum(axis=-1).astype(np.uint32) << 16))


class LadderRun:
    """N ladders resident in HBM, advanced in chunks by qecmc_pteq_resume_dev: chunked runs reproduce one long run bit for
    bit (Philox is addressed by the steps already done), so a 10^6-sweep study costs one pass, checkpoints are free, and no
    single launch runs for minutes.  Device memory through torch (plumbing).

    conv_criteria="error_based" (with SEQ, TOPS, eps; alpha for the alpha rule; scan "random" or "sweep") runs the reference's stopping
    rule instead (qecmc_pteq_resume_conv_dev): every ladder stops where the one long criterion run stops it, whatever the chunks.  The
    criterion's per-ladder records and its log live here too; the log starts with `log_rows` rows (default: the first chunk) and grows
    geometrically (grown_log_rows)."""

    def __init__(self, init, p, Nc=None, iters=10, tops_burn=2, p_logical=0.5, seed=0, first_syndrome=0, device=0,
                 code=L_.TORIC, eta=None, conv_criteria=None, SEQ=2, TOPS=10, eps=0.1, alpha=None, scan="random", log_rows=None):
        import torch
        if conv_criteria not in (None, "error_based"):
            raise ValueError(f"conv_criteria={conv_criteria!r}: only None and 'error_based' exist for PTEQ")
        a, _ = L_.as_states(init, 3 if code in (L_.TORIC, L_.PLANAR) else 2)
        self.N, size = a.shape[0], a.shape[-1]
        self.Nc = Nc or size
        self.ncls = 16 if code == L_.TORIC else 4
        self.shape = a.shape[1:]
        nq = int(np.prod(self.shape))
        self.conv = conv_criteria is not None
        noise = L_.NOISE_ALPHA if alpha is not None else L_.NOISE_DEPOLARIZING if eta is None else L_.NOISE_BIASED
        self._mk = lambda steps: L_.make_params(code=code, L=size, Nc=self.Nc, p=float(p), p_logical=float(p_logical), iters=int(iters),
                                                steps=int(steps), tops_burn=int(tops_burn), seed=seed, device=device,
                                                noise=noise, eta=float(eta or 0.0), alpha=float(alpha or 0.0), scan=L_.SCANS.get(scan, scan),
                                                conv_mode=L_.CONV_ERROR_BASED if self.conv else L_.CONV_NONE, TOPS=int(TOPS), SEQ=int(SEQ),
                                                eps=float(eps))
        self.first = int(first_syndrome)
        dev = torch.device("cuda", device)
        st = np.broadcast_to(a.reshape(self.N, 1, nq), (self.N, self.Nc, nq))            # Ladder.__init__, mcmc.py:72
        self.states = torch.from_numpy(np.array(st, order="C")).to(dev)                  # (a writable copy of the broadcast view)
        fl = np.zeros((self.N, self.Nc), dtype=np.uint8); fl[:, -1] = 1                    # mcmc.py:75
        self.flags = torch.from_numpy(fl).to(dev)
        self.tops0 = torch.zeros(self.N, dtype=torch.int32, device=dev)
        self.counts = torch.zeros((self.N, self.ncls), dtype=torch.int32, device=dev)
        self.samples = torch.zeros(self.N, dtype=torch.int32, device=dev)
        self.steps = 0
        self._plans = {}
        self._torch = torch
        if self.conv:
            self.steps_done = torch.zeros(self.N, dtype=torch.int32, device=dev)
            self.converged = torch.zeros(self.N, dtype=torch.uint8, device=dev)
            self.neff = torch.from_numpy(packed_neff(st).view(np.int32)).to(dev) if alpha is not None else None
            self.record = None                                                           # (sized by the library: the first chunk's plan knows)
            self.log = None
            self.log_rows = 0
            self._log_rows0 = None if log_rows is None else int(log_rows)

    def _plan(self, steps):
        import ctypes as C
        if steps not in self._plans:
            pl = C.c_void_p()
            L_.check(L_.lib().qecmc_plan_create(self._mk(steps), C.byref(pl)))
            self._plans[steps] = pl
        return self._plans[steps]

    def _sizes(self, plan, rows):
        import ctypes as C
        rec, log = C.c_uint64(), C.c_uint64()
        L_.check(L_.lib().qecmc_plan_resume_conv_bytes(plan, self.N, int(rows), C.byref(rec), C.byref(log)))
        return int(rec.value), int(log.value)

    def _fit_log(self, plan, steps):
        """the criterion's records (all zero: a fresh run) and a log that holds rows [0, self.steps + steps)"""
        torch, dev = self._torch, self.states.device
        if self.log is None:
            rows = max(self._log_rows0 if self._log_rows0 is not None else steps, 1)
            rec_b, log_b = self._sizes(plan, rows)
            self.record = torch.zeros(rec_b, dtype=torch.uint8, device=dev)
            self.log, self.log_rows = torch.empty(log_b, dtype=torch.uint8, device=dev), rows
        rows, keep = grown_log_rows(self.log_rows, self.steps, steps)
        if rows != self.log_rows:
            new = torch.empty(self._sizes(plan, rows)[1], dtype=torch.uint8, device=dev)
            keep_b = self._sizes(plan, keep)[1]
            new[:keep_b].copy_(self.log[:keep_b])
            self.log, self.log_rows = new, rows

    def advance(self, steps):
        import ctypes as C
        steps = int(steps)
        if steps <= 0:
            return self
        plan = self._plan(steps)
        stream = self._torch.cuda.current_stream(self.states.device)
        if self.conv:
            self._fit_log(plan, steps)
            L_.check(L_.lib().qecmc_pteq_resume_conv_dev(
                plan, self.states.data_ptr(), self.flags.data_ptr(), self.tops0.data_ptr(), self.N, self.first, self.steps,
                self.counts.data_ptr(), self.samples.data_ptr(), self.steps_done.data_ptr(), self.converged.data_ptr(),
                self.record.data_ptr(), self.record.numel(), None if self.neff is None else self.neff.data_ptr(),
                self.log.data_ptr(), self.log.numel(), self.log_rows, C.c_void_p(stream.cuda_stream)))
        else:
            L_.check(L_.lib().qecmc_pteq_resume_dev(plan, self.states.data_ptr(), self.flags.data_ptr(), self.tops0.data_ptr(),
                                                    self.N, self.first, self.steps, self.counts.data_ptr(), self.samples.data_ptr(),
                                                    C.c_void_p(stream.cuda_stream)))
        self.steps += steps
        return self

    def run_until_converged(self, max_steps, chunk):
        """Advance in chunks of `chunk` ladder steps until every ladder has converged or `max_steps` are done (criterion runs)."""
        if not self.conv:
            raise ValueError("run_until_converged needs conv_criteria='error_based'")
        max_steps, chunk = int(max_steps), int(chunk)
        if chunk <= 0:
            raise ValueError("chunk must be positive")
        while self.steps < max_steps:
            self.advance(min(chunk, max_steps - self.steps))
            if bool(self.converged.all().item()):
                break
        return self

    def snapshot(self, states=False):
        self._torch.cuda.synchronize()
        out = dict(steps=self.steps, counts=self.counts.cpu().numpy().view(np.uint32), samples=self.samples.cpu().numpy().view(np.uint32),
                   tops0=self.tops0.cpu().numpy().view(np.uint32))
        if self.conv:
            out["steps_done"] = self.steps_done.cpu().numpy().view(np.uint32)
            out["converged"] = self.converged.cpu().numpy().astype(bool)
        if states:
            out["states"] = self.states.cpu().numpy().reshape((self.N, self.Nc) + self.shape)
            out["flags"] = self.flags.cpu().numpy()
        return out

    def close(self):
        for pl in self._plans.values():
            L_.lib().qecmc_plan_destroy(pl)
        self._plans = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def convergence_study(init, p, checkpoints, Nc=None, iters=10, tops_burn=0, seed=0, code=L_.TORIC, chunk=None, **run_kw):
    """Class histograms of the same chains at increasing run lengths (BASELINE config 5: "long-chain convergence study").
    The ladders stay in HBM (LadderRun) and are advanced from checkpoint to checkpoint -- an exact continuation, so the whole
    study costs one run to the last checkpoint; `chunk` bounds the ladder steps of a single launch (default 2^20).
    Returns dict(steps int64[k], counts uint32[k, N, ncls], samples uint32[k, N], percent uint8[k, N, ncls],
    tv float64[k]) with tv = mean total-variation distance of each checkpoint's class distribution to the last one."""
    from .decoders import percent_from_counts
    cps = sorted(int(c) for c in checkpoints)
    chunk = int(chunk or (1 << 20))
    run = LadderRun(init, p, Nc=Nc, iters=iters, tops_burn=tops_burn, seed=seed, code=code, **run_kw)
    snaps = []
    for c in cps:
        while run.steps < c:
            run.advance(min(chunk, c - run.steps))
        snaps.append(run.snapshot())
    run.close()
    counts = np.stack([r["counts"] for r in snaps])
    samples = np.stack([r["samples"] for r in snaps])
    frac = counts / np.maximum(samples, 1)[..., None].astype(np.float64)
    tv = 0.5 * np.abs(frac - frac[-1]).sum(axis=-1).mean(axis=-1)
    return dict(steps=np.array(cps, dtype=np.int64), counts=counts, samples=samples, tops0=np.stack([r["tops0"] for r in snaps]),
                percent=np.stack([percent_from_counts(r["counts"], r["samples"]) for r in snaps]), tv=tv)
