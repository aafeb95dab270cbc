"""Start chains from bare syndromes (qecmc_chains_from_syndromes; no counterpart in the reference, whose decoders all start from
an error chain, generate_data.py:131).  The chain is the XOR of the rows of the code's lift table over the set defect cells -- one
Pauli string per check, found by breadth-first search over the single-qubit X / Z errors -- followed by a greedy descent over the
stabilizer generators.  No matching: a local minimum of the weight, in an arbitrary equivalence class."""
import ctypes as C
import math

import numpy as np

from . import _lib as L_

_CODES = {"toric": L_.TORIC, "xzzx": L_.XZZX, "rotated": L_.ROTATED, "planar": L_.PLANAR}


def defect_cells(code, size):
    """cells of the defect layout qecmc_syndrome writes for one syndrome"""
    code = _CODES.get(code, code)
    return 2 * size * size if code == L_.TORIC else 2 * size * (size - 1) if code == L_.PLANAR else (size + 1) * (size + 1)


def _isqrt_exact(n, what):
    r = math.isqrt(int(n)) if n >= 0 else -1
    if r * r != n:
        raise ValueError(f"{what}: {n} cells fit no system size")
    return r


def flatten_defects(code, defects, size=None):
    """defects -> (uint8[N, cells], size, batched?).  Accepts what the code classes' syndrom() / syndrome() return -- toric
    [..., 2, L, L], xzzx / rotated [..., L+1, L+1], planar the pair (vertex_defects [..., L-1, L], plaquette_defects [..., L, L-1]) --
    or the flat layout [..., cells]; a non-zero entry is a defect.  A 2-D square array of the xzzx / rotated codes is read as ONE grid
    (what syndrome() returns); give `size` to pass a flat batch of that shape."""
    code = _CODES.get(code, code)
    if code == L_.PLANAR and isinstance(defects, (tuple, list)) and len(defects) == 2 and np.ndim(defects[0]) >= 2:
        v, q = (np.asarray(x) != 0 for x in defects)
        L = v.shape[-1]
        if v.shape[-2:] != (L - 1, L) or q.shape[-2:] != (L, L - 1) or v.shape[:-2] != q.shape[:-2] or (size is not None and size != L):
            raise ValueError(f"planar defects must be (vertex [..., L-1, L], plaquette [..., L, L-1]), got {v.shape} and {q.shape}")
        batched = v.ndim == 3
        flat = np.concatenate([v.reshape(-1, (L - 1) * L), q.reshape(-1, L * (L - 1))], axis=1)
        return np.ascontiguousarray(flat, dtype=np.uint8), L, batched
    d = np.asarray(defects) != 0
    if d.ndim == 0:
        raise ValueError("defects must be an array")
    shaped = None                                            # trailing axes of the shaped layout, if that is what we were given
    if code == L_.TORIC and d.ndim >= 3 and d.shape[-3] == 2 and d.shape[-1] == d.shape[-2]:
        shaped, L = 3, d.shape[-1]
    elif code in (L_.XZZX, L_.ROTATED) and d.ndim >= 2 and d.shape[-1] == d.shape[-2] and (size is None or size + 1 == d.shape[-1]):
        shaped, L = 2, d.shape[-1] - 1
    if shaped is None:
        cells = d.shape[-1]
        if size is not None:
            L = int(size)
        elif code == L_.TORIC:
            L = _isqrt_exact(cells / 2, "toric defects")
        elif code == L_.PLANAR:
            L = (1 + _isqrt_exact(1 + 2 * cells, "planar defects")) // 2
        else:
            L = _isqrt_exact(cells, "xzzx / rotated defects") - 1
        shaped = 1
    if size is not None and size != L:
        raise ValueError(f"defects of shape {d.shape} do not belong to size {size}")
    lead = d.shape[:-shaped]
    if len(lead) > 1 or int(np.prod(d.shape[-shaped:])) != defect_cells(code, L):
        raise ValueError(f"defects of shape {d.shape} fit neither the shaped nor the flat layout of size {L}")
    return np.ascontiguousarray(d.reshape(-1, defect_cells(code, L)), dtype=np.uint8), L, len(lead) == 1


def _via_torch(code, L, flat, descend, device, nq):
    """a device other than 0: the lift is made on that device and run through the device-pointer entry point"""
    import torch
    with torch.cuda.device(device):
        dev = torch.device("cuda", device)
        d = torch.from_numpy(flat).to(dev)
        n = flat.shape[0]
        chains = torch.empty((n, nq), dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.uint8, device=dev)
        weight = torch.empty(n, dtype=torch.int32, device=dev)
        lf = C.c_void_p()
        L_.check(L_.lib().qecmc_lift_create(code, L, C.byref(lf)))
        try:
            L_.check(L_.lib().qecmc_chains_from_syndromes_dev(lf, d.data_ptr(), n, int(bool(descend)), chains.data_ptr(), status.data_ptr(),
                                                              weight.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            torch.cuda.synchronize(dev)
        finally:
            L_.lib().qecmc_lift_destroy(lf)
        return chains.cpu().numpy(), status.cpu().numpy(), weight.cpu().numpy()


def chains_from_syndromes(code, defects, descend=True, device=0, size=None):
    """One start chain per syndrome, on the GPU.  code: "toric" / "xzzx" / "rotated" / "planar" (or the qecmc code number); defects as
    flatten_defects() takes them.  descend=False returns the bare table lift.
    Returns dict(chains uint8[N, ...] shaped like the code's qubit_matrix (no leading axis for a single syndrome), status uint8[N]: 0
    lifted, 1 not a syndrome of this code (that chain is all zero), weight int32[N]: the chain's error count, -1 with status 1)."""
    code = _CODES.get(code, code)
    flat, L, batched = flatten_defects(code, defects, size)
    n = flat.shape[0]
    shape = (2, L, L) if code in (L_.TORIC, L_.PLANAR) else (L, L)
    nq = int(np.prod(shape))
    if int(device) != 0:
        chains, status, weight = _via_torch(code, L, flat, descend, int(device), nq)
    else:
        chains = np.zeros((n, nq), dtype=np.uint8)
        status = np.zeros(n, dtype=np.uint8)
        weight = np.zeros(n, dtype=np.int32)
        L_.check(L_.lib().qecmc_chains_from_syndromes(code, L, n, L_.u8(flat), int(bool(descend)), L_.u8(chains), L_.u8(status), L_.i32(weight)))
    chains = chains.reshape((n,) + shape)
    if not batched:
        return dict(chains=chains[0], status=status[0], weight=weight[0])
    return dict(chains=chains, status=status, weight=weight)
