"""Corrections from decoded syndromes (qecmc_corrections; no counterpart in the reference, which returns a class histogram).  Given
candidate chains with a syndrome and the class the decoder chose, the kernel returns a chain with that syndrome IN that class: the
lightest candidate already there, else the lightest of all moved by logical operators -- each placed where it costs least -- and then
the lift's greedy descent."""
import ctypes as C

import numpy as np

from . import _lib as L_

_CODES = {"toric": L_.TORIC, "xzzx": L_.XZZX, "rotated": L_.ROTATED, "planar": L_.PLANAR}


def _as_candidates(code, candidates, size):
    """candidates -> (uint8[N, K, nq], state shape).  [N, K, ...] or [N, ...] (K = 1) with ... the code's qubit_matrix shape; with `size`
    given also the flat layouts [N, K, nq] and [N, nq]."""
    a = np.ascontiguousarray(candidates, dtype=np.uint8)
    sd = 3 if code in (L_.TORIC, L_.PLANAR) else 2
    if size is not None and a.ndim in (2, 3) and a.shape[-1] == (2 if sd == 3 else 1) * size * size:
        L, lead = int(size), a.shape[:-1]
    else:
        if a.ndim not in (sd + 1, sd + 2) or a.shape[-1] != a.shape[-2] or (sd == 3 and a.shape[-3] != 2) or (size is not None and size != a.shape[-1]):
            raise ValueError(f"candidates of shape {a.shape} are neither [N, K, ...] nor [N, ...] configurations of this code" +
                             ("" if size is None else f" at size {size}"))
        L, lead = a.shape[-1], a.shape[:-sd]
    shape = (2, L, L) if sd == 3 else (L, L)
    n, k = (lead[0], 1) if len(lead) == 1 else lead
    if k < 1:
        raise ValueError("a correction needs at least one candidate chain per syndrome")
    return a.reshape(n, k, int(np.prod(shape))), shape


def _via_torch(code, L, cand, target, place, descend, device):
    """a device other than 0: the corrector is made on that device and run through the device-pointer entry point"""
    import torch
    with torch.cuda.device(device):
        dev = torch.device("cuda", device)
        n, k, nq = cand.shape
        d_c, d_t = torch.from_numpy(cand).to(dev), torch.from_numpy(target).to(dev)
        out = torch.empty((n, nq), dtype=torch.uint8, device=dev)
        weight, source = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        moved, status = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2))
        cr = C.c_void_p()
        L_.check(L_.lib().qecmc_corrector_create(code, L, C.byref(cr)))
        try:
            L_.check(L_.lib().qecmc_corrections_dev(cr, d_c.data_ptr(), d_t.data_ptr(), n, k, int(bool(place)), int(bool(descend)), out.data_ptr(),
                                                    weight.data_ptr(), source.data_ptr(), moved.data_ptr(), status.data_ptr(),
                                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            torch.cuda.synchronize(dev)
        finally:
            L_.lib().qecmc_corrector_destroy(cr)
        return tuple(x.cpu().numpy() for x in (out, weight, source, moved, status))


def corrections(code, candidates, target, place=True, descend=True, device=0, size=None):
    """One correction per syndrome, on the GPU.  code: "toric" / "xzzx" / "rotated" / "planar" (or the qecmc code number); candidates
    uint8[N, K, ...] or [N, ...] (K = 1): chains that all have the syndrome (not checked); target int[N]: the class the correction shall
    lie in (the column order of counts / distr).  place=False puts every logical operator of a class move at position 0, descend=False
    skips the greedy descent.
    Returns dict(corrections uint8[N, ...], weight int32[N]: the error count, source int32[N]: the candidate it came from, moved uint8[N]:
    1 iff no candidate was in the target class, status uint8[N]: 0 corrected, 1 target outside [0, ncls) -- that chain is all zero,
    weight -1, source -1)."""
    code = _CODES.get(code, code)
    cand, shape = _as_candidates(code, candidates, size)
    n, k, nq = cand.shape
    tgt = np.ascontiguousarray(np.broadcast_to(np.asarray(target), (n,)), dtype=np.int32)
    if int(device) != 0:
        out, weight, source, moved, status = _via_torch(code, shape[-1], cand, tgt, place, descend, int(device))
    else:
        out = np.zeros((n, nq), dtype=np.uint8)
        weight, source = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        moved, status = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        L_.check(L_.lib().qecmc_corrections(code, shape[-1], n, k, L_.u8(cand), L_.i32(tgt), int(bool(place)), int(bool(descend)), L_.u8(out),
                                            L_.i32(weight), L_.i32(source), L_.u8(moved), L_.u8(status)))
    return dict(corrections=out.reshape((n,) + shape), weight=weight, source=source, moved=moved, status=status)
