"""Guard zones around the buffers handed to a library entry.  Not a test file, no fixtures; its own
negative controls are in tests/test_guarded.py.

``guarded(payload, role, guard_bytes)`` makes ONE allocation ``[guard | payload | guard]`` on the
payload's device (torch) or on the host (numpy), fills it, and returns the payload view and a handle;
``check(handles)`` looks at the bits afterwards.  A guard is ``guard_bytes(nbytes, batch)`` =
max(4096, 8 × the array's bytes per trajectory) rounded up to a multiple of 256 bytes, so every
payload keeps the 256-byte alignment of a fresh device allocation.

Fill:
  role "in"     guards hold a quiet NaN with a recognisable payload (fp64 0x7FF8DEADBEEFCAFE,
                fp32 0x7FC0BEEF; int32 0x5A5A5A5A, bytes 0x5A); the payload holds the caller's data
  role "out"    guards AND payload hold that pattern
  role "inout"  like "in" (NaN guards, real payload); only the guards are checked
  role "ws"     a workspace: an "out" of exactly the reported bytes of which only the guards are
                checked (what a library leaves in its workspace is its own business)

``check`` compares integer views, after a device synchronise:
  (a) every guard of every array, inputs included, is bit-identical to its fill;
  (b) every element of every "out" payload differs from the fill pattern and, for a floating type,
      is finite — except the elements the handle's ``unspecified`` mask names (what include/lqrx.h
      declares unspecified, handed in by the test).
A failure names the array, the side, and the first and last offending element counted from the
payload's edge: before the payload −1 is the element that touches it, after it 0 is.

What this can see and what it cannot.  A store outside the payload changes a guard.  A load outside
an input that reaches the result carries the NaN into an output, which (b) reports — 0 · NaN is NaN,
so a padded operand "multiplied away" is seen as well — or at least changes the result's bits
against a run on plain tensors, which the tests compare.  A load whose value is discarded (an
unused prefetch past a buffer) leaves no trace and is NOT seen; neither is anything past the far
end of a guard.  Misaligned payloads are not tested either: the ABI promises nothing about
alignment, and an unaligned pointer on a shared GPU is not something to find out by trying.
"""
import numpy as np

F64_PATTERN = 0x7FF8DEADBEEFCAFE
F32_PATTERN = 0x7FC0BEEF
I32_PATTERN = 0x5A5A5A5A
BYTE_PATTERN = 0x5A
ROLES = ("in", "out", "inout", "ws")


class GuardError(AssertionError):
    pass


def guard_bytes(nbytes: int, batch: int) -> int:
    """max(4096, 8 × bytes per trajectory), rounded up to a multiple of 256."""
    g = max(4096, 8 * (-(-int(nbytes) // max(1, int(batch)))))
    return -(-g // 256) * 256


def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


def _int_view_of(dtype_name: str):
    """payload dtype name → (numpy integer dtype of the same width, fill pattern, is_float)"""
    return {"float64": (np.int64, F64_PATTERN, True), "float32": (np.int32, F32_PATTERN, True),
            "int32": (np.int32, I32_PATTERN, False), "uint8": (np.uint8, BYTE_PATTERN, False)}[dtype_name]


class Handle:
    """One guarded array: `full` is the whole allocation as integers, `view` the payload in the
    caller's type and shape, `g` the elements of each guard, `unspecified` an optional boolean mask
    (flat, payload-sized; numpy) of elements (b) skips."""

    def __init__(self, name, role, full, view, g, size, pattern, is_float):
        self.name, self.role, self.full, self.view = name, role, full, view
        self.g, self.size, self.pattern, self.is_float = g, size, pattern, is_float
        self.unspecified = None

    def host_bits(self):
        f = self.full
        return f.cpu().numpy() if _is_torch(f) else f


def guarded(payload, role: str, guard_bytes: int, name: str = ""):
    """payload: a torch tensor or numpy array (float64, float32, int32 or uint8, contiguous) — its
    data for "in" / "inout", only its shape, type and device for "out" / "ws".  Returns
    (view, handle): the view has the payload's shape and type and lies between two guards of
    `guard_bytes` bytes each inside one allocation."""
    if role not in ROLES:
        raise ValueError(f"guarded: role {role!r}, expected one of {ROLES}")
    tor = _is_torch(payload)
    dname = str(payload.dtype).replace("torch.", "")
    idt, pattern, is_float = _int_view_of(dname)
    item = np.dtype(idt).itemsize
    if guard_bytes % 256 or guard_bytes <= 0:
        raise ValueError("guarded: guard_bytes must be a positive multiple of 256")
    g = guard_bytes // item
    size = int(payload.numel() if tor else payload.size)
    if tor:
        import torch

        tdt = {np.int64: torch.int64, np.int32: torch.int32, np.uint8: torch.uint8}[idt]
        full = torch.full((2 * g + size,), pattern, dtype=tdt, device=payload.device)
        view = full[g:g + size].view(payload.dtype).view(payload.shape)
        if role in ("in", "inout"):
            view.copy_(payload)
    else:
        full = np.full(2 * g + size, pattern, dtype=idt)
        view = full[g:g + size].view(payload.dtype).reshape(payload.shape)
        if role in ("in", "inout"):
            view[...] = payload
    return view, Handle(name or role, role, full, view, g, size, pattern, is_float)


def guard_all(arrays: dict, role: str, batch: int, handles: list, prefix: str = "") -> dict:
    """guarded() over a dict of arrays (entries that are not arrays pass through): returns the dict
    of views and appends the handles to `handles`."""
    out = {}
    for k, a in arrays.items():
        if not (hasattr(a, "dtype") and hasattr(a, "shape") and len(a.shape) >= 1):
            out[k] = a
            continue
        nbytes = (a.numel() * a.element_size()) if _is_torch(a) else a.nbytes
        out[k], h = guarded(a, role, guard_bytes(nbytes, batch), prefix + k)
        handles.append(h)
    return out


def _span(idx):
    return int(idx[0]), int(idx[-1])


def problems(handles) -> list:
    """Every violation of (a) and (b) as a line of text; empty when all is well."""
    hs = list(handles.values()) if isinstance(handles, dict) else list(handles)
    if any(_is_torch(h.full) and h.full.is_cuda for h in hs):
        import torch

        torch.cuda.synchronize()
    msgs = []
    for h in hs:
        bits = h.host_bits()
        pat = bits.dtype.type(h.pattern)
        lo, mid, hi = bits[:h.g], bits[h.g:h.g + h.size], bits[h.g + h.size:]
        bad = np.flatnonzero(lo != pat)
        if bad.size:
            a, b = _span(bad - h.g)
            msgs.append(f"{h.name} ({h.role}): guard BEFORE the payload overwritten, {bad.size} element(s), "
                        f"offsets {a} .. {b} from the payload's first element")
        bad = np.flatnonzero(hi != pat)
        if bad.size:
            a, b = _span(bad)
            msgs.append(f"{h.name} ({h.role}): guard AFTER the payload overwritten, {bad.size} element(s), "
                        f"offsets {a} .. {b} past the payload's last element")
        if h.role != "out":
            continue
        keep = np.ones(h.size, bool) if h.unspecified is None else ~np.asarray(h.unspecified, bool).reshape(-1)
        bad = np.flatnonzero((mid == pat) & keep)
        if bad.size:
            a, b = _span(bad)
            msgs.append(f"{h.name} (out): payload NOT WRITTEN (still the fill pattern: skipped, or the NaN of an input's guard carried here), {bad.size} element(s), "
                        f"offsets {a} .. {b} from the payload's first element")
        if h.is_float:
            val = mid.view(np.float64 if mid.dtype == np.int64 else np.float32)
            bad = np.flatnonzero(~np.isfinite(val) & (mid != pat) & keep)
            if bad.size:
                a, b = _span(bad)
                msgs.append(f"{h.name} (out): payload NOT FINITE, {bad.size} element(s), "
                            f"offsets {a} .. {b} from the payload's first element")
    return msgs


def check(handles) -> None:
    """Raises GuardError (an AssertionError) listing every violation of (a) and (b)."""
    msgs = problems(handles)
    if msgs:
        raise GuardError("guard check failed:\n  " + "\n  ".join(msgs))


def pattern_filled(shape_like, n: int | None = None):
    """A plain exact-size tensor / array like `shape_like` (or of n elements of its type and device)
    holding the fill pattern instead of whatever the allocator hands back."""
    tor = _is_torch(shape_like)
    dname = str(shape_like.dtype).replace("torch.", "")
    idt, pattern, _ = _int_view_of(dname)
    size = int(n if n is not None else (shape_like.numel() if tor else shape_like.size))
    if tor:
        import torch

        tdt = {np.int64: torch.int64, np.int32: torch.int32, np.uint8: torch.uint8}[idt]
        return torch.full((size,), pattern, dtype=tdt, device=shape_like.device).view(shape_like.dtype)
    return np.full(size, pattern, dtype=idt).view(shape_like.dtype)
