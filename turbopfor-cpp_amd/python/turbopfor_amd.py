"""Python host binding of libturbopfor_amd.so (ctypes over the C-ABI in
include/turbopfor_gpu.h).  Device buffers are torch tensors on a HIP device;
kernels run on torch's current stream.  There is no CPU fallback: every
entry point raises if the HIP library or device is missing.

Reference interface mirrored: include/turbopfor.h of amosbird/TurboPFor-CPP
(per-block p4Enc*/p4Dec*), lifted to batches of blocks with explicit byte
offsets (the reference's callers chain blocks through the returned pointer).
"""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.dirname(_HERE)
# TPF_LIB: load another build of the library (A/B measurements only)
LIB_PATH = os.environ.get("TPF_LIB") or os.path.join(PKG_DIR, "lib", "libturbopfor_amd.so")

_lib = None

c_u64 = ctypes.c_uint64
c_vp = ctypes.c_void_p


class TpfError(RuntimeError):
    pass


def build():
    subprocess.check_call(["make", "-s", "-C", PKG_DIR, f"-j{min(os.cpu_count() or 4, 16)}"])


def _md5(files, root):
    import hashlib

    h = hashlib.md5()
    for f in sorted(files):
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def source_md5():
    """md5 over the library's sources (turbopfor-cpp_amd/csrc/*, its Makefile
    and include/*.h, sorted by path; path and contents): the identity of the
    build (build_stamp.json).  (The built .so's own bytes differ when the same
    sources are rebuilt elsewhere -- e.g. a build on the GPU box embeds that
    box's paths -- so they do not identify the code.)"""
    root = os.path.dirname(PKG_DIR)
    files = [os.path.join(PKG_DIR, "Makefile")]
    for d in (os.path.join(PKG_DIR, "csrc"), os.path.join(root, "include")):
        files += [os.path.join(d, f) for f in os.listdir(d) if f.endswith((".h", ".hip", ".cpp"))]
    return _md5(files, root)


def kernel_md5():
    """md5 over the DEVICE code only (csrc/*.hip, csrc/*.h, the Makefile's
    flags): the identity of the kernels a PMC traffic measurement was taken
    with.  Host-side edits (host_api.cpp, host_stream.cpp, include/) do not
    change what a kernel moves, so they do not invalidate the measurement."""
    root = os.path.dirname(PKG_DIR)
    d = os.path.join(PKG_DIR, "csrc")
    files = [os.path.join(PKG_DIR, "Makefile")] + [os.path.join(d, f) for f in os.listdir(d) if f.endswith((".h", ".hip"))]
    return _md5(files, root)


# ---- the C ABI, read from the headers that state it -------------------------
HEADERS = tuple(os.path.join(os.path.dirname(PKG_DIR), "include", h) for h in ("turbopfor_gpu.h", "turbopfor_capi.h"))
_C_TYPES = {"uint64_t": c_u64, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t,
            "int": ctypes.c_int, "unsigned": ctypes.c_uint}
_C_WORDS = set(_C_TYPES) | {"void", "char", "short", "long", "signed", "float", "double"}


def _c_type(decl, where, ret=False):
    """The ctypes type of one parameter (with or without its name) or of a
    return type: the table of prototypes(), nothing beyond it."""
    words = decl.replace("*", " * ").split()
    if "*" in words:
        return ctypes.c_char_p if ret and words == ["const", "char", "*"] else c_vp
    words = [w for w in words if w != "const"]
    if not ret and len(words) == 2 and re.fullmatch(r"[A-Za-z_]\w*", words[1]) and words[1] not in _C_WORDS:
        words.pop()  # the parameter's name
    if len(words) == 1 and (words[0] in _C_TYPES or (ret and words[0] == "void")):
        return _C_TYPES.get(words[0])
    raise TpfError(f"{where}: no ctypes type for '{' '.join(decl.split())}'")


def prototypes(headers=HEADERS):
    """{name: (restype, [argtypes])} of every tpf_* function the public
    headers declare (tpfm_* of the measurement library's header), read from the
    headers themselves (comments and preprocessor lines stripped), so that
    nothing restates the ABI by hand.  Pointer parameters are c_void_p;
    uint64_t, int64_t, uint32_t, size_t, int and unsigned their ctypes
    namesakes; a void return is None, a const char * return c_char_p, any
    other pointer return c_void_p.  Strict: a type outside that table, a tpf_
    declaration this parse cannot read or a missing header raises TpfError
    naming the file and the declaration."""
    protos = {}
    for path in headers:
        try:
            with open(path) as f:
                text = f.read()
        except OSError as e:
            raise TpfError(f"{path}: header not found ({e})")
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
        text = re.sub(r'extern\s+"C"\s*\{', "", text)
        for stmt in text.split(";"):
            if not re.search(r"\btpfm?_\w+\s*\(", stmt):
                continue
            where = f"{path}: '{' '.join(stmt.split())}'"
            m = re.fullmatch(r"\s*([\w\s*]+?)\b(tpfm?_\w+)\s*\(([^()]*)\)\s*", stmt)
            if not m:
                raise TpfError(f"{where}: not a prototype this parse reads")
            ret, name, params = m.groups()
            params = [] if params.strip() == "void" else params.split(",")
            protos[name] = (_c_type(ret, where, ret=True), [_c_type(p, where) for p in params])
    return protos


def declare(L, protos=None):
    """Give every function of protos (default: prototypes()) that the loaded
    ctypes.CDLL L exports its restype and argtypes; returns L.  Symbols L lacks
    are skipped (an older build loaded through TPF_LIB for an A/B run).  No
    torch."""
    for name, (restype, argtypes) in (protos or prototypes()).items():
        if hasattr(L, name):
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    return L


def lib():
    """Load (building if needed) the in-tree HIP library."""
    global _lib
    if _lib is None:
        # torch bundles its own libamdhip64 (soname libamdhip64.so.7, file
        # name libamdhip64.so).  Load it first so our library binds to that
        # same HIP runtime instead of a second copy from /opt/rocm.
        import torch  # noqa: F401

        if not os.path.exists(LIB_PATH):
            build()
        _lib = declare(ctypes.CDLL(LIB_PATH))
    return _lib


def _check(rc):
    if rc != 0:
        raise TpfError(f"turbopfor_amd error {rc}: {lib().tpf_last_error().decode()}")


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _index(packed, offsets, list_ptr, list_unit):
    """The arguments every call on a resident lists index begins with: packed,
    its length, offsets, nunits, list_ptr, list_unit, nlists."""
    return (_ptr(packed), packed.numel(), _ptr(offsets), offsets.numel() - 1, _ptr(list_ptr), _ptr(list_unit),
            list_ptr.numel() - 1)


def _ws(ws, device, size_export, *counts):
    """The workspace of a call: the caller's ws when it holds the bytes
    size_export(*counts) asks for, else a fresh uint8 tensor of that size (of
    1 byte for a size of 0) on device."""
    size = int(size_export(*counts))
    if ws is None or ws.numel() < size:
        import torch

        ws = torch.empty(max(size, 1), dtype=torch.uint8, device=device)
    return ws


def dec256v32(packed, offsets, nblocks, out=None, starts=None, err=None):
    """Decode nblocks 256v32 blocks.  packed: uint8 CUDA tensor; offsets:
    int64 CUDA tensor [nblocks+1]; starts: optional int32 [nblocks] for the
    delta-1 variant (p4D1Dec256v32).  Returns int32 tensor [nblocks, 256]
    (bit pattern = uint32)."""
    import torch

    if out is None:
        out = torch.empty((nblocks, 256), dtype=torch.int32, device=packed.device)
    L = lib()
    if starts is None:
        rc = L.tpf_p4dec256v32_batch(_ptr(packed), packed.numel(), _ptr(offsets), nblocks, _ptr(out), _ptr(err),
                                     _stream(torch))
    else:
        rc = L.tpf_p4d1dec256v32_batch(_ptr(packed), packed.numel(), _ptr(offsets), nblocks, _ptr(out),
                                       _ptr(starts), _ptr(err), _stream(torch))
    _check(rc)
    return out


# ---- the measurement / test library (measure/tpf_measure.h) --------------
# Not the codec: kernel probes, device ceilings, forced encoder paths and the
# run-scan test hook, loaded only by bench.py, the GPU tests and scripts/.
MEASURE_PATH = os.path.join(PKG_DIR, "lib", "libtpf_measure.so")
_mlib = None


def measure():
    """Load lib/libtpf_measure.so (after the codec library it links)."""
    global _mlib
    if _mlib is None:
        lib()
        if not os.path.exists(MEASURE_PATH):
            build()
        _mlib = declare(ctypes.CDLL(MEASURE_PATH), prototypes([os.path.join(PKG_DIR, "measure", "tpf_measure.h")]))
    return _mlib


def _mcheck(rc, what):
    if rc != 0:
        raise TpfError(f"{what}: measurement library error {rc}")


def probe256v64(packed, offsets, nunits, out):
    """Measurement only: the 256v64 decode kernel's loads and stores without
    the decoding (tpfm_probe256v64)."""
    import torch

    _mcheck(measure().tpfm_probe256v64(_ptr(packed), packed.numel(), _ptr(offsets), nunits, _ptr(out), _stream(torch)),
            "tpfm_probe256v64")
    return out


def probe256v32(packed, offsets, nblocks, out):
    """Measurement only: the decode kernel's loads and stores without the
    decoding (data-movement ceiling of the hot path's access pattern)."""
    import torch

    _mcheck(measure().tpfm_probe256v32(_ptr(packed), packed.numel(), _ptr(offsets), nblocks, _ptr(out), _stream(torch)),
            "tpfm_probe256v32")
    return out


def dec256v32_path(grouped, packed, offsets, nblocks, out):
    """Measurement only: the plain 256v32 decode through a forced load path
    (tpfm_dec256v32_path: grouped 0 = single-block pipeline, 1 = grouped 1 KB
    loads; the library chooses per launch)."""
    import torch

    _mcheck(measure().tpfm_dec256v32_path(1 if grouped else 0, _ptr(packed), packed.numel(), _ptr(offsets), nblocks, _ptr(out),
                                          _stream(torch)), "tpfm_dec256v32_path")
    return out


def probe_hbm(kind, dst, src, nbytes):
    """Measurement only: streaming ceiling kernels (tpfm_probe_hbm): kind
    "read" (src), "write" (dst) or "copy" (src -> dst) of nbytes bytes."""
    import torch

    k = {"read": 0, "write": 1, "copy": 2}[kind]
    _mcheck(measure().tpfm_probe_hbm(k, _ptr(dst), _ptr(src), nbytes, _stream(torch)), "tpfm_probe_hbm")


def enc256v32_path(mode, values, out, d1=False, starts=None, start0=0):
    """The 256v32 encoder through a forced path (tpfm_enc256v32): mode 1 =
    plan pass as a wave OR, 2 = write pass copying values (plain only, not a
    valid stream), 3 = the two-pass encoder (the library's), 4 / 5 = the slot
    encoder with / without the fused scans (measured, not adopted).  Returns
    the offsets tensor [nblocks+1]."""
    import torch

    nb = values.numel() // 256
    offs = torch.empty(nb + 1, dtype=torch.int64, device=values.device)
    ws_bytes = int(measure().tpfm_enc256v32_workspace_size(mode, nb))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=values.device)
    _mcheck(measure().tpfm_enc256v32(mode, _ptr(values), nb, 1 if d1 else 0, _ptr(starts), ctypes.c_uint32(start0 & 0xFFFFFFFF),
                                     _ptr(out), out.numel(), _ptr(offs), _ptr(ws), ws_bytes, _stream(torch)), "tpfm_enc256v32")
    return offs


def enc256v32(values, d1=False, starts=None, start0=0, out=None, offs=None, ws=None):
    """Encode values (int32/uint32-bit CUDA tensor, nblocks*256 elements) as
    256v32 P4 blocks.  Returns (packed uint8 tensor sized to the encoded
    total, offsets int64 tensor [nblocks+1]).  d1 selects p4D1Enc256v32:
    starts (int32 [nblocks]) gives each block's preceding value, or with
    starts=None the blocks form one chained list starting after start0.
    out / offs / ws: optional preallocated buffers (out's numel() is the
    capacity, ws's the workspace size); with out and offs both given the call
    stays asynchronous and returns out untrimmed."""
    import torch

    assert values.is_cuda and values.dtype in (torch.int32,) and values.numel() % 256 == 0
    values = values.contiguous()
    nb = values.numel() // 256
    L = lib()
    trim = out is None or offs is None
    if out is None:
        out = torch.empty(int(L.tpf_p4enc256v32_bound(nb)), dtype=torch.uint8, device=values.device)
    if offs is None:
        offs = torch.empty(nb + 1, dtype=torch.int64, device=values.device)
    ws = _ws(ws, values.device, L.tpf_p4enc256v32_workspace_size, nb)
    if d1:
        rc = L.tpf_p4d1enc256v32_batch(_ptr(values), nb, _ptr(starts), ctypes.c_uint32(start0 & 0xFFFFFFFF),
                                       _ptr(out), out.numel(), _ptr(offs), _ptr(ws), ws.numel(), _stream(torch))
    else:
        rc = L.tpf_p4enc256v32_batch(_ptr(values), nb, _ptr(out), out.numel(), _ptr(offs), _ptr(ws), ws.numel(),
                                     _stream(torch))
    _check(rc)
    if not trim:
        return out, offs
    total = int(offs[-1].item())
    return out[:total], offs


# ---- every turbopfor.h family (include/turbopfor_gpu.h tpf_{enc,dec}_batch) ----
FMT = {"32": 0, "128v32": 1, "256v32": 2, "64": 3, "128v64": 4, "256v64": 5}
_WIDE = {"64", "128v64", "256v64"}
_UNIT = {"128v32": 128, "256v32": 256, "128v64": 128, "256v64": 256}


def unit_values(fmt, n):
    return _UNIT.get(fmt, n)


def enc_batch(fmt, values, nblocks, n, d1=False, starts=None, start0=0, out=None, offs=None, ws=None):
    """values: int32/int64 CUDA tensor with nblocks*unit_values(fmt, n)
    elements (bit patterns of uint32/uint64).  Returns (packed, offsets).
    out / offs / ws: optional preallocated buffers (reused across calls)."""
    import torch

    values = values.contiguous()
    assert values.numel() == nblocks * unit_values(fmt, n)
    L = lib()
    f = FMT[fmt]
    cap = int(L.tpf_enc_bound(f, nblocks, n))
    if out is None:
        out = torch.empty(cap, dtype=torch.uint8, device=values.device)
    assert out.numel() >= cap
    cap = out.numel()
    if offs is None:
        offs = torch.empty(nblocks + 1, dtype=torch.int64, device=values.device)
    ws = _ws(ws, values.device, L.tpf_enc_workspace_size, f, nblocks, n)
    rc = L.tpf_enc_batch(f, _ptr(values), nblocks, n, 1 if d1 else 0, _ptr(starts),
                         ctypes.c_uint64(start0 & ((1 << 64) - 1)), _ptr(out), cap, _ptr(offs), _ptr(ws), ws.numel(),
                         _stream(torch))
    _check(rc)
    return out[: int(offs[-1].item())], offs


def dec_batch(fmt, packed, offsets, nblocks, n, starts=None, err=None, out=None):
    import torch

    dt = torch.int64 if fmt in _WIDE else torch.int32
    if out is None:
        out = torch.zeros(nblocks * unit_values(fmt, n), dtype=dt, device=packed.device)
    L = lib()
    rc = L.tpf_dec_batch(FMT[fmt], _ptr(packed), packed.numel(), _ptr(offsets), nblocks, n, _ptr(out), _ptr(starts),
                         _ptr(err), _stream(torch))
    _check(rc)
    return out


# ---- chained delta-1 decode of one posting list (f1) ----------------------
class D1Chain:
    """Two-phase chained p4D1Dec256v32 over one list: sums() decodes every
    block's delta sum and its prefix (returns the shard total as a 1-element
    int32 CUDA tensor), decode(base) writes the values.  A multi-GPU list
    runs sums() on every shard, exchanges the totals, then decode() with
    base = start0 + sum of earlier shards' totals (mod 2^32).  ws / total:
    optional caller's workspace (its numel() is the size passed) and
    1-element int32 total."""

    def __init__(self, packed, offsets, nblocks, ws=None, total=None):
        import torch

        self.packed, self.offsets, self.nblocks = packed, offsets, nblocks
        L = lib()
        ws = _ws(ws, packed.device, L.tpf_p4d1dec256v32_chain_workspace_size, nblocks)
        self.ws, self.ws_bytes = ws, ws.numel()
        self.total = torch.zeros(1, dtype=torch.int32, device=packed.device) if total is None else total

    def sums(self, err=None):
        import torch

        rc = lib().tpf_p4d1dec256v32_chain_sums(_ptr(self.packed), self.packed.numel(), _ptr(self.offsets), self.nblocks,
                                                _ptr(self.ws), self.ws_bytes, _ptr(self.total), _ptr(err),
                                                _stream(torch))
        _check(rc)
        return self.total

    def decode(self, base, out=None, err=None):
        import torch

        if out is None:
            out = torch.empty((self.nblocks, 256), dtype=torch.int32, device=self.packed.device)
        rc = lib().tpf_p4d1dec256v32_chain_decode(_ptr(self.packed), self.packed.numel(), _ptr(self.offsets),
                                                  self.nblocks, _ptr(out), ctypes.c_uint32(base & 0xFFFFFFFF),
                                                  _ptr(self.ws), _ptr(err), _stream(torch))
        _check(rc)
        return out


class D1Chain64:
    """The 64-bit counterpart of D1Chain over one chained list of fmt "256v64"
    or "128v64" units (tpf_d1dec64_chain_sums / tpf_d1dec64_chain_decode):
    sums() returns the shard total as a 1-element int64 CUDA tensor (mod
    2^64), decode(base) writes int64 [nunits, 256 or 128].  ws / total:
    optional caller's workspace (its numel() is the size passed) and
    1-element int64 total."""

    def __init__(self, fmt, packed, offsets, nunits, ws=None, total=None):
        import torch

        self.fmt, self.width = FMT[fmt], _UNIT[fmt]
        self.packed, self.offsets, self.nunits = packed, offsets, nunits
        ws = _ws(ws, packed.device, lib().tpf_d1dec64_chain_workspace_size, nunits)
        self.ws, self.ws_bytes = ws, ws.numel()
        self.total = torch.zeros(1, dtype=torch.int64, device=packed.device) if total is None else total

    def sums(self, err=None):
        import torch

        _check(lib().tpf_d1dec64_chain_sums(self.fmt, _ptr(self.packed), self.packed.numel(), _ptr(self.offsets), self.nunits,
                                            _ptr(self.ws), self.ws_bytes, _ptr(self.total), _ptr(err), _stream(torch)))
        return self.total

    def decode(self, base, out=None, err=None):
        import torch

        if out is None:
            out = torch.empty((self.nunits, self.width), dtype=torch.int64, device=self.packed.device)
        _check(lib().tpf_d1dec64_chain_decode(self.fmt, _ptr(self.packed), self.packed.numel(), _ptr(self.offsets), self.nunits,
                                              _ptr(out), ctypes.c_uint64(base & 0xFFFFFFFFFFFFFFFF), _ptr(self.ws), _ptr(err),
                                              _stream(torch)))
        return out


def dec256v32_chained(packed, offsets, nblocks, start0=0, out=None, err=None, ws=None):
    """One chained list (block i starts from block i-1's last value, block 0
    from start0): tpf_p4d1dec256v32_chained (block sums + scan, then decode).
    ws: optional reusable uint8 workspace tensor."""
    import torch

    if out is None:
        out = torch.empty((nblocks, 256), dtype=torch.int32, device=packed.device)
    L = lib()
    ws = _ws(ws, packed.device, L.tpf_p4d1dec256v32_chain_workspace_size, nblocks)
    rc = L.tpf_p4d1dec256v32_chained(_ptr(packed), packed.numel(), _ptr(offsets), nblocks, _ptr(out),
                                     ctypes.c_uint32(start0 & 0xFFFFFFFF), _ptr(ws), ws.numel(), _ptr(err),
                                     _stream(torch))
    _check(rc)
    return out


def dec64_chained(fmt, packed, offsets, nunits, start0=0, out=None, err=None, ws=None, named=False):
    """One chained 64-bit list of fmt "256v64" or "128v64" units (unit i
    starts from unit i-1's last value, unit 0 from start0): tpf_d1dec64_chained
    (unit sums + scan, then decode), or with named=True the format's own entry
    point tpf_p4d1dec256v64_chained / tpf_p4d1dec128v64_chained.  Returns
    int64 [nunits, 256 or 128]."""
    import torch

    width = _UNIT[fmt]
    if out is None:
        out = torch.empty((nunits, width), dtype=torch.int64, device=packed.device)
    L = lib()
    ws = _ws(ws, packed.device, L.tpf_d1dec64_chain_workspace_size, nunits)
    args = (_ptr(packed), packed.numel(), _ptr(offsets), nunits, _ptr(out), ctypes.c_uint64(start0 & 0xFFFFFFFFFFFFFFFF), _ptr(ws),
            ws.numel(), _ptr(err), _stream(torch))
    rc = getattr(L, f"tpf_p4d1dec{fmt}_chained")(*args) if named else L.tpf_d1dec64_chained(FMT[fmt], *args)
    _check(rc)
    return out


# ---- n-variant streams (include/turbopfor_gpu.h tpf_p4nenc256v32) ----------
def n_units(n):
    """Blocks in an n-value stream: n // 256 256v32 blocks + one p4Enc32 tail."""
    return n // 256 + (1 if n % 256 else 0)


def encn256v32(values, d1=False, start0=0, out=None, offs=None, ws=None):
    """Encode any number of int32 values as the stream the reference produces
    by chaining p4Enc256v32 over the full 256-blocks and p4Enc32 over the
    remainder (p4D1* with d1, one list starting after start0).  Returns
    (packed uint8 tensor, offsets int64 [n_units(n) + 1]).  out / offs / ws:
    optional preallocated buffers (out's numel() is the capacity, ws's the
    workspace size); with out and offs both given the call stays asynchronous
    and returns out untrimmed."""
    import torch

    assert values.is_cuda and values.dtype == torch.int32
    values = values.contiguous().view(-1)
    n = values.numel()
    L = lib()
    trim = out is None or offs is None
    if out is None:
        out = torch.empty(int(L.tpf_p4nenc256v32_bound(n)), dtype=torch.uint8, device=values.device)
    if offs is None:
        offs = torch.empty(n_units(n) + 1, dtype=torch.int64, device=values.device)
    ws = _ws(ws, values.device, L.tpf_p4nenc256v32_workspace_size, n)
    _check(L.tpf_p4nenc256v32(_ptr(values), n, int(bool(d1)), ctypes.c_uint32(start0 & 0xFFFFFFFF), _ptr(out), out.numel(),
                              _ptr(offs), _ptr(ws), ws.numel(), _stream(torch)))
    if not trim:
        return out, offs
    return out[:int(offs[-1].item())], offs


def decn256v32(packed, offsets, n, d1=False, start0=0, out=None, err=None, ws=None):
    """Decode an n-value stream of encn256v32's layout (offsets: n_units(n)+1).
    ws: optional reusable uint8 workspace tensor (its numel() is the size
    passed)."""
    import torch

    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=packed.device)
    L = lib()
    ws = _ws(ws, packed.device, L.tpf_p4ndec256v32_workspace_size, n)
    _check(L.tpf_p4ndec256v32(_ptr(packed), packed.numel(), _ptr(offsets), n, int(bool(d1)),
                              ctypes.c_uint32(start0 & 0xFFFFFFFF), _ptr(out), _ptr(ws), ws.numel(), _ptr(err),
                              _stream(torch)))
    return out


# ---- many lists in one call (include/turbopfor_gpu.h tpf_p4ndec256v32_lists) ----
def lists_units(list_ptr):
    """Per-list unit counts and unit bases of a lists stream: list j of
    n_j = list_ptr[j+1] - list_ptr[j] values holds n_units(n_j) units starting
    at unit base[j].  list_ptr: a CPU tensor, numpy array or sequence of
    nlists + 1 non-decreasing integers.  Returns (units, base) as int64 numpy
    arrays of nlists and nlists + 1 entries (base[nlists] = the stream's unit
    count).  Pure host code: the library is not loaded."""
    import numpy as np

    if hasattr(list_ptr, "detach"):
        list_ptr = list_ptr.detach().cpu().numpy()
    p = np.asarray(list_ptr).astype(np.int64).reshape(-1)
    if p.size == 0:
        raise ValueError("list_ptr holds nlists + 1 entries")
    n = np.diff(p)
    if (n < 0).any():
        raise ValueError("list_ptr must be non-decreasing")
    units = n // 256 + (n % 256 != 0)
    base = np.zeros(p.size, dtype=np.int64)
    np.cumsum(units, out=base[1:])
    return units.astype(np.int64), base


def decn256v32_lists(packed, offsets, list_ptr, d1=False, start0=None, out=None, err=None, ws=None):
    """Decode many lists laid end to end in one call: list j is an
    encn256v32-layout stream of list_ptr[j+1] - list_ptr[j] values, its units
    following list j-1's; offsets: int64 [nunits + 1].  list_ptr: int64 CUDA
    tensor [nlists + 1] (CSR form); start0: optional int32 CUDA tensor
    [nlists] of each list's preceding value (d1 only; None = 0).  out: int32
    CUDA tensor whose numel() is the capacity in values (default: sized from
    list_ptr[-1], which costs a device-to-host read; pass out to stay
    asynchronous).  Values land at out[list_ptr[j]:list_ptr[j+1]]."""
    import torch

    nlists = list_ptr.numel() - 1
    nunits = offsets.numel() - 1
    if out is None:
        out = torch.empty(int(list_ptr[-1].item()), dtype=torch.int32, device=packed.device)
    L = lib()
    ws = _ws(ws, packed.device, L.tpf_p4ndec256v32_lists_workspace_size, nunits, nlists)
    _check(L.tpf_p4ndec256v32_lists(_ptr(packed), packed.numel(), _ptr(offsets), nunits, _ptr(list_ptr), nlists, int(bool(d1)),
                                    _ptr(start0), _ptr(out), out.numel(), _ptr(ws), ws.numel(), _ptr(err), _stream(torch)))
    return out


# ---- many lists in one call, encode (include/turbopfor_gpu.h tpf_p4nenc256v32_lists) ----
def lists_enc_bound(nvalues, nlists):
    """A capacity in bytes that always suffices for encn256v32_lists of
    nvalues values in nlists lists (tpf_p4nenc256v32_lists_bound: advice, not a
    precondition -- the device checks the real length against the capacity)."""
    return int(lib().tpf_p4nenc256v32_lists_bound(int(nvalues), int(nlists)))


def encn256v32_lists(values, list_ptr, d1=False, start0=None, nunits=None, out=None, offsets=None, err=None, ws=None):
    """Encode many lists laid end to end in one call: list j is
    values[list_ptr[j]:list_ptr[j+1]] and becomes an encn256v32-layout stream,
    the streams concatenated in list order -- what decn256v32_lists reads.
    values: int32 CUDA tensor (its numel() is the readable length); list_ptr:
    int64 CUDA tensor [nlists + 1] (CSR form); start0: optional int32 CUDA
    tensor [nlists] of each list's preceding value (d1 only; None = 0).
    nunits: the stream's unit count (default: computed from list_ptr with
    lists_units, which costs a device-to-host read).  out: uint8 CUDA tensor
    whose numel() is the capacity (default: lists_enc_bound bytes, trimmed to
    offsets[-1], which costs another read); offsets: int64 CUDA tensor
    [nunits + 1]; err: optional int64 CUDA tensor [1] (-1 = clean).  With
    nunits, out and offsets all given the call stays asynchronous and returns
    out untrimmed.  Returns (packed, offsets)."""
    import torch

    assert values.is_cuda and values.dtype == torch.int32
    values = values.contiguous().view(-1)
    nlists = list_ptr.numel() - 1
    if nunits is None:
        nunits = int(lists_units(list_ptr)[1][-1])
    trim = out is None
    if out is None:
        nvalues = int(list_ptr[-1].item()) - int(list_ptr[0].item()) if nlists > 0 else 0
        out = torch.empty(max(lists_enc_bound(nvalues, nlists), 1), dtype=torch.uint8, device=values.device)
    if offsets is None:
        offsets = torch.empty(nunits + 1, dtype=torch.int64, device=values.device)
    L = lib()
    ws = _ws(ws, values.device, L.tpf_p4nenc256v32_lists_workspace_size, nunits, nlists)
    _check(L.tpf_p4nenc256v32_lists(_ptr(values), values.numel(), _ptr(list_ptr), nlists, int(bool(d1)), _ptr(start0), _ptr(out),
                                    out.numel(), _ptr(offsets), nunits, _ptr(ws), ws.numel(), _ptr(err), _stream(torch)))
    if trim:
        out = out[:int(offsets[nunits].item())]
    return out, offsets


# ---- the read side of a resident index (include/turbopfor_gpu.h tpf_p4ndec256v32_lists_select) ----
def lists_unit_base(list_ptr, out=None, err=None, ws=None):
    """The unit directory of a lists stream, on the device: out[j] = the first
    unit of list j, out[nlists] = the stream's unit count (the device form of
    lists_units(list_ptr)[1]).  list_ptr: int64 CUDA tensor [nlists + 1]; out:
    int32 CUDA tensor [nlists + 1]; err: optional int64 CUDA tensor [1] (-1 =
    clean; j: list_ptr decreases at j; nlists: more than 0x7FFFFFFF units).
    Asynchronous: no device-to-host read."""
    import torch

    nlists = list_ptr.numel() - 1
    if out is None:
        out = torch.empty(nlists + 1, dtype=torch.int32, device=list_ptr.device)
    L = lib()
    ws = _ws(ws, list_ptr.device, L.tpf_lists_unit_base_workspace_size, nlists)
    _check(L.tpf_lists_unit_base(_ptr(list_ptr), nlists, _ptr(out), _ptr(ws), ws.numel(), _ptr(err), _stream(torch)))
    return out


def decn256v32_lists_select(packed, offsets, list_ptr, list_unit, sel, d1=False, start0=None, out=None, out_ptr=None, err=None,
                            ws=None):
    """Decode lists sel[0 .. nsel) of a resident lists stream, in the order
    given, into one dense output: selection k lands at
    out[out_ptr[k]:out_ptr[k+1]].  packed / offsets / list_ptr: the stream as
    decn256v32_lists reads it; list_unit: int32 CUDA tensor [nlists + 1] from
    lists_unit_base; sel: int32 CUDA tensor of list ids, any order, repeats
    allowed; start0: optional int32 CUDA tensor [nlists], indexed by the lists
    of the index (d1 only; None = 0).  out: int32 CUDA tensor whose numel() is
    the capacity in values -- pass one sized for the selection, not for the
    index: the work is sized by it (default: sized from list_ptr and sel, which
    costs a device-to-host read; pass out to stay asynchronous).  out_ptr:
    int64 CUDA tensor [nsel + 1], written; err: optional int64 CUDA tensor [1]
    (-1 = clean).  Returns (out, out_ptr)."""
    import torch

    nlists = list_ptr.numel() - 1
    nsel = sel.numel()
    if out is None:
        total = 0
        if nsel and nlists > 0:
            idx = sel.long() & 0xFFFFFFFF
            ok = idx < nlists
            idx = idx.clamp(max=nlists - 1)
            total = int(((list_ptr[idx + 1] - list_ptr[idx]).clamp(min=0) * ok).sum().item())
        out = torch.empty(max(total, 1), dtype=torch.int32, device=packed.device)[:total]
    if out_ptr is None:
        out_ptr = torch.empty(nsel + 1, dtype=torch.int64, device=packed.device)
    L = lib()
    ws = _ws(ws, packed.device, L.tpf_p4ndec256v32_lists_select_workspace_size, nsel, out.numel())
    _check(L.tpf_p4ndec256v32_lists_select(*_index(packed, offsets, list_ptr, list_unit), int(bool(d1)), _ptr(start0), _ptr(sel), nsel,
                                           _ptr(out), out.numel(), _ptr(out_ptr), _ptr(ws), ws.numel(), _ptr(err), _stream(torch)))
    return out, out_ptr


# ---- block-range reads of a resident index (include/turbopfor_gpu.h tpf_lists_unit_last,
# tpf_lists_range_units, tpf_p4ndec256v32_lists_units) ----
def lists_unit_last(packed, offsets, list_ptr, start0=None, out=None, err=None, ws=None):
    """The skip table of a delta-1 lists stream, on the device, once per
    index: out[u] = the last decoded value of unit u (mod 2^32), tails
    included.  packed / offsets / list_ptr / start0: the stream as
    decn256v32_lists reads it with d1=True; out: int32 CUDA tensor [nunits];
    err: optional int64 CUDA tensor [1] (-1 = clean; reported as
    decn256v32_lists reports).  The index is not decoded into a value-sized
    buffer.  Asynchronous: no device-to-host read."""
    import torch

    nlists = list_ptr.numel() - 1
    nunits = offsets.numel() - 1
    if out is None:
        out = torch.empty(nunits, dtype=torch.int32, device=packed.device)
    L = lib()
    ws = _ws(ws, packed.device, L.tpf_lists_unit_last_workspace_size, nunits, nlists)
    _check(L.tpf_lists_unit_last(_ptr(packed), packed.numel(), _ptr(offsets), nunits, _ptr(list_ptr), nlists, _ptr(start0), _ptr(out),
                                 _ptr(ws), ws.numel(), _ptr(err), _stream(torch)))
    return out


def lists_range_units(list_unit, unit_last, qlist, qlo, qhi, ufirst=None, ucount=None, err=None):
    """Doc-id ranges to unit ranges: query k asks for the units of list
    qlist[k] that can hold a value in [qlo[k], qhi[k]] (inclusive; the int32
    tensors are read as uint32).  list_unit: int32 CUDA tensor [nlists + 1]
    from lists_unit_base; unit_last: int32 CUDA tensor [nunits] from
    lists_unit_last.  ufirst / ucount: int32 CUDA tensors [nq], written:
    list-relative first unit and unit count, (0, 0) when nothing can match;
    err: optional int64 CUDA tensor [1] (-1 = clean; k: the first query with
    a bad list id, which gets (0, 0)).  qlist, ufirst and ucount feed
    decn256v32_lists_units unchanged.  Asynchronous.  Returns (ufirst,
    ucount)."""
    import torch

    nlists = list_unit.numel() - 1
    nunits = unit_last.numel()
    nq = qlist.numel()
    if ufirst is None:
        ufirst = torch.empty(nq, dtype=torch.int32, device=qlist.device)
    if ucount is None:
        ucount = torch.empty(nq, dtype=torch.int32, device=qlist.device)
    _check(lib().tpf_lists_range_units(_ptr(list_unit), _ptr(unit_last), nlists, nunits, _ptr(qlist), _ptr(qlo), _ptr(qhi), nq,
                                       _ptr(ufirst), _ptr(ucount), _ptr(err), _stream(torch)))
    return ufirst, ucount


def decn256v32_lists_units(packed, offsets, list_ptr, list_unit, sel, ufirst, ucount, d1=False, start0=None, unit_last=None, out=None,
                           out_ptr=None, err=None, ws=None):
    """Decode units [ufirst[k], ufirst[k] + ucount[k]) of list sel[k] of a
    resident lists stream, for every k in the order given, into one dense
    output: selection k lands at out[out_ptr[k]:out_ptr[k+1]] -- 256 values
    per unit, n % 256 in the list's tail unit.  packed / offsets / list_ptr /
    list_unit / sel / start0: as decn256v32_lists_select; ufirst, ucount: int32
    CUDA tensors [nsel] (from lists_range_units, or any ranges inside the
    lists); unit_last: the skip table of lists_unit_last, required with d1
    (every unit starts from the table: each selected block is decoded once)
    and ignored without.  out: int32 CUDA tensor whose numel() is the capacity
    in values -- the work is sized by it (default: sized from the ranges, which
    costs a device-to-host read; pass out to stay asynchronous).  out_ptr:
    int64 CUDA tensor [nsel + 1], written; err: optional int64 CUDA tensor [1]
    (-1 = clean).  Returns (out, out_ptr)."""
    import torch

    nlists = list_ptr.numel() - 1
    nsel = sel.numel()
    if out is None:
        total = 0
        if nsel and nlists > 0:
            idx = sel.long() & 0xFFFFFFFF
            uf, uc = ufirst.long() & 0xFFFFFFFF, ucount.long() & 0xFFFFFFFF
            ok = idx < nlists
            idx = idx.clamp(max=nlists - 1)
            n = (list_ptr[idx + 1] - list_ptr[idx]).clamp(min=0)
            units = (n + 255) // 256
            ok = ok & (uf + uc <= units)
            reach = (uc > 0) & (uf + uc == units) & (n % 256 != 0)
            total = int(((256 * uc - reach * (256 - n % 256)) * ok).sum().item())
        out = torch.empty(max(total, 1), dtype=torch.int32, device=packed.device)[:total]
    if out_ptr is None:
        out_ptr = torch.empty(nsel + 1, dtype=torch.int64, device=packed.device)
    L = lib()
    ws = _ws(ws, packed.device, L.tpf_p4ndec256v32_lists_units_workspace_size, nsel, out.numel())
    _check(L.tpf_p4ndec256v32_lists_units(*_index(packed, offsets, list_ptr, list_unit), int(bool(d1)), _ptr(start0), _ptr(unit_last),
                                          _ptr(sel), _ptr(ufirst), _ptr(ucount), nsel, _ptr(out), out.numel(), _ptr(out_ptr), _ptr(ws),
                                          ws.numel(), _ptr(err), _stream(torch)))
    return out, out_ptr


# ---- opening a stream without offsets (include/turbopfor_gpu.h tpf_lists_unit_offsets,
# include/turbopfor_capi.h tpf_lists_scan_offsets) ----
LISTS_SCAN_RUN = 16     # kScanRun (csrc/p4_lists_scan.hip): lists per wave of the walk
LISTS_SCAN_WINDOW = 1024  # kScanWin: bytes of the stream the walker holds in LDS


def lists_unit_offsets(packed, list_ptr, list_byte, nunits=None, out=None, list_unit=None, err=None, ws=None):
    """The unit offsets of a lists stream that has none, on the device, once
    per index: out[list_unit[j] + i] = the byte offset of unit i of list j and
    out[nunits] = list_byte[nlists], from the lists' byte spans and the units'
    own headers.  packed: uint8 CUDA tensor; list_ptr / list_byte: int64 CUDA
    tensors [nlists + 1] -- list j holds list_ptr[j+1] - list_ptr[j] values in
    the bytes [list_byte[j], list_byte[j+1]) of packed.  nunits: the stream's
    unit count (default: from out, else computed from list_ptr with
    lists_units, which costs a device-to-host read).  out: int64 CUDA tensor
    [nunits + 1]; list_unit: optional int32 CUDA tensor [nlists + 1], written
    as lists_unit_base writes it; err: optional int64 CUDA tensor [1] (-1 =
    clean; the codes of tpf_lists_unit_offsets).  Asynchronous when nunits or
    out is given.  Returns out."""
    import torch

    nlists = list_ptr.numel() - 1
    if nunits is None:
        nunits = out.numel() - 1 if out is not None else int(lists_units(list_ptr)[1][-1])
    if out is None:
        out = torch.empty(nunits + 1, dtype=torch.int64, device=packed.device)
    L = lib()
    ws = _ws(ws, packed.device, L.tpf_lists_unit_offsets_workspace_size, nunits, nlists)
    _check(L.tpf_lists_unit_offsets(_ptr(packed), packed.numel(), _ptr(list_ptr), _ptr(list_byte), nlists, _ptr(out), nunits,
                                    _ptr(list_unit), _ptr(ws), ws.numel(), _ptr(err), _stream(torch)))
    return out


def lists_scan_offsets_host(packed, list_ptr, list_byte=None, nunits=None):
    """The same on the host, sequentially (tpf_lists_scan_offsets): the
    definition lists_unit_offsets is held to, which also serves a stream
    without per-list anchors.  packed: bytes or a uint8 numpy array; list_ptr:
    nlists + 1 integers; list_byte: nlists + 1 integers, or None for lists that
    lie end to end from byte 0.  Returns (offsets, code): offsets an int64
    numpy array [nunits + 1], code -1 when clean, else the call's code."""
    import numpy as np

    buf = np.frombuffer(packed, dtype=np.uint8) if isinstance(packed, (bytes, bytearray, memoryview)) else np.ascontiguousarray(packed, np.uint8)
    ptr = np.ascontiguousarray(list_ptr, dtype=np.uint64)
    lb = None if list_byte is None else np.ascontiguousarray(list_byte, dtype=np.uint64)
    if nunits is None:
        nunits = int(lists_units(np.asarray(list_ptr))[1][-1])
    off = np.zeros(nunits + 1, dtype=np.uint64)
    r = lib().tpf_lists_scan_offsets(buf.ctypes.data, buf.size, ptr.ctypes.data, ptr.size - 1, None if lb is None else lb.ctypes.data,
                                     off.ctypes.data, nunits)
    return off.astype(np.int64), (-1 if r >= 0 else -r - 1)


def lists_list_byte(offsets, list_unit):
    """list_byte of a resident index: offsets[list_unit[j]] for j = 0 ..
    nlists, the first byte of every list and the stream's end -- what a saver
    keeps when it drops the 8 bytes per unit of offsets, and what
    lists_unit_offsets takes to rebuild them.  A torch gather on the tensors'
    device."""
    return offsets[list_unit.long()]


# ---- intersection with a resident index (include/turbopfor_gpu.h tpf_lists_intersect) ----
def _lists_probe(op, packed, offsets, list_ptr, list_unit, unit_last, probe, probe_ptr, qlist, start0, out, out_ptr, pidx, tpos, err, ws):
    """The body of lists_intersect, lists_union and lists_difference: the
    three entry points take the same arguments, and only the union's workspace
    is sized by out as well."""
    import torch

    nq = qlist.numel()
    if out is None:
        out = torch.empty(probe.numel(), dtype=torch.int32, device=packed.device)
    if out_ptr is None:
        out_ptr = torch.empty(nq + 1, dtype=torch.int64, device=packed.device)
    L = lib()
    sized_by = (nq, probe.numel(), out.numel()) if op == "union" else (nq, probe.numel())
    ws = _ws(ws, packed.device, getattr(L, f"tpf_lists_{op}_workspace_size"), *sized_by)
    _check(getattr(L, f"tpf_lists_{op}")(*_index(packed, offsets, list_ptr, list_unit), _ptr(start0), _ptr(unit_last), _ptr(probe),
                                         probe.numel(), _ptr(probe_ptr), _ptr(qlist), nq, _ptr(out), out.numel(), _ptr(out_ptr),
                                         _ptr(pidx), _ptr(tpos), _ptr(ws), ws.numel(), _ptr(err), _stream(torch)))
    return out, out_ptr


def lists_intersect(packed, offsets, list_ptr, list_unit, unit_last, probe, probe_ptr, qlist, start0=None, out=None, out_ptr=None,
                    pidx=None, tpos=None, err=None, ws=None):
    """Which probe doc ids are in their target lists: query k is the values
    probe[probe_ptr[k]:probe_ptr[k+1]] (int32 CUDA tensor read as uint32,
    sorted for the least work; probe_ptr: int64 CUDA tensor [nq + 1],
    non-decreasing) tested against list qlist[k] (int32 CUDA tensor [nq]) of a
    resident delta-1 lists stream.  packed / offsets / list_ptr / list_unit /
    start0: as decn256v32_lists_units with d1=True; unit_last: the skip table
    of lists_unit_last.  The hits of query k land at
    out[out_ptr[k]:out_ptr[k+1]] in probe order, so (out, out_ptr) is the
    probe of the next call of a k-term AND.  Only the blocks a probe value
    lands in are decoded, and none is written to memory.  out: int32 CUDA
    tensor whose numel() is the capacity in values (default: probe.numel(),
    which always suffices, so the default stays asynchronous); out_ptr: int64
    CUDA tensor [nq + 1], written; pidx / tpos: optional int32 CUDA tensors of
    out's capacity, written when passed: the hit's index into probe and its
    position in the target list; err: optional int64 CUDA tensor [1] (-1 =
    clean).  Returns (out, out_ptr)."""
    return _lists_probe("intersect", packed, offsets, list_ptr, list_unit, unit_last, probe, probe_ptr, qlist, start0, out, out_ptr, pidx,
                        tpos, err, ws)


# ---- union with a resident index (include/turbopfor_gpu.h tpf_lists_union) ----
LISTS_NONE = 0xFFFFFFFF  # TPF_LISTS_NONE: pidx of a value the probe does not hold, tpos of one the list does not hold


def lists_union(packed, offsets, list_ptr, list_unit, unit_last, probe, probe_ptr, qlist, start0=None, out=None, out_ptr=None,
                pidx=None, tpos=None, err=None, ws=None):
    """The sorted union of probe doc ids with their target lists: query k is
    the strictly ascending values probe[probe_ptr[k]:probe_ptr[k+1]] (int32
    CUDA tensor read as uint32; probe_ptr: int64 CUDA tensor [nq + 1],
    non-decreasing) merged with list qlist[k] (int32 CUDA tensor [nq]) of a
    resident delta-1 lists stream.  packed / offsets / list_ptr / list_unit /
    start0 / unit_last: as lists_intersect.  The union of query k lands at
    out[out_ptr[k]:out_ptr[k+1]], ascending, so (out, out_ptr) is the probe of
    the next call of a k-term OR; the first probe is a decn256v32_lists_select
    decode.  out: int32 CUDA tensor whose numel() is the capacity in values,
    REQUIRED: a capacity that always suffices is probe.numel() plus the lengths
    of the targeted lists, which lie in list_ptr on the device, and reading
    them back would synchronise -- the caller, who built the index, knows them
    (err == nunits + nq: out_ptr[nq] is what to allocate).  out_ptr: int64
    CUDA tensor [nq + 1], written; pidx / tpos: optional int32 CUDA tensors of
    out's capacity, written when passed: the index into probe of a value the
    probe holds and the position in the target list of a value the list holds,
    LISTS_NONE otherwise; err: optional int64 CUDA tensor [1] (-1 = clean).
    The workspace is allocated here unless ws is large enough.  Asynchronous:
    no device-to-host read.  Returns (out, out_ptr)."""
    if out is None:
        raise ValueError("lists_union: out is required (its numel() is the capacity; sizing it here would read list_ptr back)")
    return _lists_probe("union", packed, offsets, list_ptr, list_unit, unit_last, probe, probe_ptr, qlist, start0, out, out_ptr, pidx, tpos,
                        err, ws)


# ---- difference with a resident index (include/turbopfor_gpu.h tpf_lists_difference) ----
def lists_difference(packed, offsets, list_ptr, list_unit, unit_last, probe, probe_ptr, qlist, start0=None, out=None, out_ptr=None,
                     pidx=None, tpos=None, err=None, ws=None):
    """Which probe doc ids are NOT in their target lists (AND NOT): query k is
    the values probe[probe_ptr[k]:probe_ptr[k+1]] (int32 CUDA tensor read as
    uint32, sorted for the least work; probe_ptr: int64 CUDA tensor [nq + 1],
    non-decreasing) tested against list qlist[k] (int32 CUDA tensor [nq]) of a
    resident delta-1 lists stream.  The arguments, defaults and allocation
    rules are lists_intersect's.  The values list qlist[k] does not hold land
    at out[out_ptr[k]:out_ptr[k+1]] in probe order, so (out, out_ptr) is the
    probe of the next lists_intersect, lists_union or lists_difference.  out:
    int32 CUDA tensor whose numel() is the capacity in values (default:
    probe.numel(), which always suffices, so the default stays asynchronous);
    out_ptr: int64 CUDA tensor [nq + 1], written; pidx / tpos: optional int32
    CUDA tensors of out's capacity, written when passed: the value's index
    into probe, and the number of list values below it -- the position of the
    first list value above it, or the list's length when there is none (not a
    lists_gather position); err: optional int64 CUDA tensor [1] (-1 = clean).
    Returns (out, out_ptr)."""
    return _lists_probe("difference", packed, offsets, list_ptr, list_unit, unit_last, probe, probe_ptr, qlist, start0, out, out_ptr, pidx,
                        tpos, err, ws)


# ---- values at list positions of a resident index (include/turbopfor_gpu.h tpf_lists_gather) ----
def lists_gather(packed, offsets, list_ptr, list_unit, pos, pos_ptr, qlist, d1=False, start0=None, unit_last=None, out=None, err=None,
                 ws=None):
    """The values at given positions of resident lists: query k is the
    list-relative positions pos[pos_ptr[k]:pos_ptr[k+1]] (int32 CUDA tensor
    read as uint32, in any order, repeats allowed, sorted for the least work;
    pos_ptr: int64 CUDA tensor [nq + 1], non-decreasing) of list qlist[k]
    (int32 CUDA tensor [nq]), and out[i] is the value at pos[i].  packed /
    offsets / list_ptr / list_unit / start0: as decn256v32_lists_units;
    unit_last: the skip table of lists_unit_last, required with d1 and ignored
    without, so the directory of a doc-id stream also serves the plain
    frequency stream stored in parallel.  (tpos, out_ptr, qlist) of
    lists_intersect are (pos, pos_ptr, qlist) here, unchanged.  Only the
    blocks a position names are decoded, and none is written to memory.  out:
    int32 CUDA tensor parallel to pos (default: torch.empty_like(pos));
    entries outside [pos_ptr[0], pos_ptr[nq]) are left alone.  err: optional
    int64 CUDA tensor [1] (-1 = clean).  Asynchronous: no device-to-host
    read.  Returns out."""
    import torch

    if d1 and unit_last is None:
        raise ValueError("lists_gather: d1=True needs unit_last (lists_unit_last)")
    nq = qlist.numel()
    if out is None:
        out = torch.empty_like(pos)
    L = lib()
    ws = _ws(ws, packed.device, L.tpf_lists_gather_workspace_size, nq, pos.numel())
    _check(L.tpf_lists_gather(*_index(packed, offsets, list_ptr, list_unit), int(bool(d1)), _ptr(start0), _ptr(unit_last), _ptr(pos),
                              pos.numel(), _ptr(pos_ptr), _ptr(qlist), nq, _ptr(out), _ptr(ws), ws.numel(), _ptr(err), _stream(torch)))
    return out


# ---- postings appended to a resident index (include/turbopfor_gpu.h tpf_lists_append) ----
LISTS_APPEND_TILE = 16384  # bytes of the output one wave of the append's stitch pass moves

# The caps of the lists launchers (csrc/p4_lists_host.h, p4_lists_dev.h, p4_lists_intersect.hip, p4_lists_gather.hip,
# p4_dec_run.h), restated for the tests that have to cross them; tests/test_lists_scale_cpu.py holds them against the sources.
LISTS_FLAT_WG_PER_CU = 8  # flat_grid: workgroups of 256 threads per CU of a grid-stride plan / heads kernel
LISTS_MIN_W = 7           # kListsMinW: workgroups per CU of the item decodes k_ix_dec / k_ga_dec
LISTS_IX_RUN = 4          # kIxRun: items per wave and trip of k_ix_dec
LISTS_GA_RUN = 4          # kGaRun: items per wave and trip of k_ga_dec
LISTS_RUN_DEFAULT = 16    # kRunDefault: units, lists, selections or items per wave of the other decodes


def _lists_cus(device):
    import torch

    return int(torch.cuda.get_device_properties(device).multi_processor_count)


def lists_flat_cap(device):
    """Threads of the largest grid flat_grid launches on `device`: a plan or
    heads kernel over more entries than this takes a second trip of its
    grid-stride loop."""
    return LISTS_FLAT_WG_PER_CU * 256 * _lists_cus(device)


def lists_item_cap(device, run=LISTS_IX_RUN):
    """Items one trip of k_ix_dec / k_ga_dec covers on `device` (4 waves per
    workgroup, `run` items per wave): a request of more items makes every wave
    stride."""
    return LISTS_MIN_W * _lists_cus(device) * 4 * run


def _index_out(dev, nlists_out, d1, out, out_offsets, units_cap, units_bound, bytes_bound):
    """The output side lists_append and lists_remove share: the caller's out /
    out_offsets / units_cap or their defaults (units_bound() and bytes_bound()
    are asked only for a default), and the new index's fresh list_ptr,
    list_unit and -- with d1 -- unit_last.  Returns the five tensors the call
    returns, and their arguments in the entry points' order."""
    import torch

    if units_cap is None:
        units_cap = out_offsets.numel() - 1 if out_offsets is not None else units_bound()
    if out_offsets is None:
        out_offsets = torch.empty(units_cap + 1, dtype=torch.int64, device=dev)
    if out is None:
        out = torch.empty(max(bytes_bound(), 1), dtype=torch.uint8, device=dev)
    list_ptr_out = torch.empty(nlists_out + 1, dtype=torch.int64, device=dev)
    list_unit_out = torch.empty(nlists_out + 1, dtype=torch.int32, device=dev)
    unit_last_out = torch.empty(max(units_cap, 1), dtype=torch.int32, device=dev) if d1 else None
    return ((out, out_offsets, list_ptr_out, list_unit_out, unit_last_out),
            (_ptr(out), out.numel(), _ptr(out_offsets), units_cap, _ptr(list_ptr_out), _ptr(list_unit_out), _ptr(unit_last_out)))


def lists_append_units_bound(nunits, nlists_out, add_values):
    """A unit capacity that always suffices for lists_append
    (tpf_lists_append_units_bound: advice, not a precondition)."""
    return int(lib().tpf_lists_append_units_bound(int(nunits), int(nlists_out), int(add_values)))


def lists_append_bound(in_bytes, nlists_out, add_values):
    """A byte capacity that always suffices for lists_append
    (tpf_lists_append_bound: advice, not a precondition)."""
    return int(lib().tpf_lists_append_bound(int(in_bytes), int(nlists_out), int(add_values)))


def lists_append(packed, offsets, list_ptr, list_unit, add, add_ptr, d1=False, start0=None, unit_last=None, nlists=None, out=None,
                 out_offsets=None, units_cap=None, err=None, ws=None, stream=None):
    """Append postings to the lists of a resident index, out of place: list j
    of the result is the old list j followed by add[add_ptr[j]:add_ptr[j+1]].
    packed / offsets / list_ptr / list_unit / start0 / unit_last: the old
    index as decn256v32_lists_units reads it (unit_last required with d1); any
    of the first four may be None for an empty old index.  nlists: the old
    index's list count (default: list_ptr.numel() - 1); add_ptr: int64 CUDA
    tensor [nlists_out + 1], nlists_out >= nlists -- lists past the old index
    are new; start0 has nlists_out entries.  add: int32 CUDA tensor.  Full
    blocks of the old stream are moved as bytes; only the tail of a list that
    receives values is decoded and encoded again, so the result is byte for
    byte encn256v32_lists of the concatenated lists.  out: uint8 CUDA tensor
    whose numel() is the byte capacity (default: lists_append_bound);
    out_offsets: int64 CUDA tensor [units_cap + 1] (default units_cap:
    lists_append_units_bound, or out_offsets.numel() - 1).  err: optional
    int64 CUDA tensor [1] (-1 = clean).  stream: a raw HIP stream handle
    (default: torch's current stream).  Asynchronous: no device-to-host
    read; the stream's length is out_offsets[list_unit_out[-1]].  Returns
    (out, out_offsets, list_ptr_out, list_unit_out, unit_last_out or None)."""
    import torch

    if d1 and unit_last is None and packed is not None and offsets is not None and offsets.numel() > 1:
        raise ValueError("lists_append: d1=True needs unit_last (lists_unit_last)")
    dev = add_ptr.device
    if nlists is None:
        nlists = list_ptr.numel() - 1 if list_ptr is not None else 0
    nunits = offsets.numel() - 1 if offsets is not None and nlists > 0 else 0
    in_bytes = packed.numel() if packed is not None else 0
    nlists_out = add_ptr.numel() - 1
    nadd = add.numel() if add is not None else 0
    L = lib()
    res, res_args = _index_out(dev, nlists_out, d1, out, out_offsets, units_cap, lambda: lists_append_units_bound(nunits, nlists_out, nadd),
                               lambda: lists_append_bound(in_bytes, nlists_out, nadd))
    ws = _ws(ws, dev, L.tpf_lists_append_workspace_size, nunits, nlists_out, nadd)
    _check(L.tpf_lists_append(_ptr(packed), in_bytes, _ptr(offsets), nunits, _ptr(list_ptr), _ptr(list_unit), nlists, int(bool(d1)),
                              _ptr(start0), _ptr(unit_last), _ptr(add), nadd, _ptr(add_ptr), nlists_out, *res_args, _ptr(ws), ws.numel(),
                              _ptr(err), stream if stream is not None else _stream(torch)))
    return res


# ---- postings deleted from a resident index (include/turbopfor_gpu.h tpf_lists_remove) ----
def lists_remove_bound(in_bytes, nq, stage_values):
    """A byte capacity that always suffices for lists_remove
    (tpf_lists_remove_bound: advice, not a precondition)."""
    return int(lib().tpf_lists_remove_bound(int(in_bytes), int(nq), int(stage_values)))


def lists_remove(packed, offsets, list_ptr, list_unit, pos, pos_ptr, qlist, stage_values, d1=False, start0=None, unit_last=None,
                 out=None, out_offsets=None, units_cap=None, err=None, ws=None, stream=None):
    """Delete the postings at list positions of a resident index, out of
    place: list qlist[k] of the result is the old list without the values at
    positions pos[pos_ptr[k]:pos_ptr[k+1]] (strictly ascending; qlist strictly
    ascending).  The tpos / out_ptr / qlist of lists_intersect feed it
    unchanged.  packed / offsets / list_ptr / list_unit / start0 / unit_last:
    the old index as decn256v32_lists_units reads it (unit_last required with
    d1).  The units of a list before its first removed position, and every
    list that loses nothing, are moved as bytes; only the suffix is decoded,
    compacted and encoded again, so the result is byte for byte
    encn256v32_lists of the shortened lists.  stage_values: the capacity of
    the staged suffixes (the sum of the targeted lists' lengths always
    suffices).  out: uint8 CUDA tensor whose numel() is the byte capacity
    (default: lists_remove_bound); out_offsets: int64 CUDA tensor [units_cap +
    1] (default units_cap: the old unit count, which always suffices).  err:
    optional int64 CUDA tensor [1] (-1 = clean).  stream: a raw HIP stream
    handle (default: torch's current stream).  Asynchronous: no
    device-to-host read; the stream's length is
    out_offsets[list_unit_out[-1]].  Returns (out, out_offsets, list_ptr_out,
    list_unit_out, unit_last_out or None)."""
    import torch

    if d1 and unit_last is None and offsets is not None and offsets.numel() > 1:
        raise ValueError("lists_remove: d1=True needs unit_last (lists_unit_last)")
    dev = list_ptr.device
    nlists = list_ptr.numel() - 1
    nunits = offsets.numel() - 1 if offsets is not None and nlists > 0 else 0
    in_bytes = packed.numel() if packed is not None else 0
    nq = qlist.numel() if qlist is not None else 0
    npos = pos.numel() if pos is not None else 0
    stage_values = int(stage_values)
    L = lib()
    res, res_args = _index_out(dev, nlists, d1, out, out_offsets, units_cap, lambda: nunits,
                               lambda: lists_remove_bound(in_bytes, nq, stage_values))
    ws = _ws(ws, dev, L.tpf_lists_remove_workspace_size, nunits, nlists, nq, npos, stage_values)
    _check(L.tpf_lists_remove(_ptr(packed), in_bytes, _ptr(offsets), nunits, _ptr(list_ptr), _ptr(list_unit), nlists, int(bool(d1)),
                              _ptr(start0), _ptr(unit_last), _ptr(pos), npos, _ptr(pos_ptr), _ptr(qlist), nq, stage_values, *res_args,
                              _ptr(ws), ws.numel(), _ptr(err), stream if stream is not None else _stream(torch)))
    return res


# ---- a sub-index of a resident index (include/turbopfor_gpu.h tpf_lists_extract) ----
def lists_extract(packed, offsets, list_ptr, list_unit, sel, ufirst=None, ucount=None, d1=False, start0=None, unit_last=None, out=None,
                  out_offsets=None, units_cap=None, err=None, ws=None, stream=None):
    """A sub-index of a resident index, moved as bytes: list k of the result
    is units [ufirst[k], ufirst[k] + ucount[k]) of list sel[k] (all of it with
    ufirst=None), in the order given; repeats get a copy each.  packed /
    offsets / list_ptr / list_unit / start0 / unit_last: the index as
    decn256v32_lists_units reads it (unit_last required with d1 and ufirst,
    optional otherwise); sel / ufirst / ucount: int32 CUDA tensors [nsel], the
    arguments of decn256v32_lists_units -- qlist and the results of
    lists_range_units feed the call unchanged.  Nothing is decoded: for an
    index this library encoded the result is byte for byte encn256v32_lists of
    the selected values with start0_out.  The frequency stream stored in
    parallel is extracted by the same selection with d1=False.  out: uint8
    CUDA tensor whose numel() is the byte capacity; out_offsets: int64 CUDA
    tensor [units_cap + 1] (default units_cap: out_offsets.numel() - 1).  With
    repeats the result can outgrow the index, so no capacity follows from the
    sizes: when units_cap (or out_offsets) or out is not given, the selection's
    unit and byte totals are summed on the device and read back, which costs a
    device-to-host read -- the only synchronous path; pass out and out_offsets
    (or units_cap) to stay asynchronous, and size them with a call on an empty
    out (err = nunits + nsel + 1 and out_offsets[list_unit_out[-1]] bytes to
    allocate).  err: optional int64 CUDA tensor [1] (-1 = clean).  stream: a
    raw HIP stream handle (default: torch's current stream).  Returns (out,
    out_offsets, list_ptr_out, list_unit_out, start0_out or None,
    unit_last_out or None); unit_last_out is None without d1 or unit_last."""
    import torch

    if d1 and ufirst is not None and unit_last is None:
        raise ValueError("lists_extract: d1=True with unit ranges needs unit_last (lists_unit_last)")
    dev = sel.device
    nlists = list_ptr.numel() - 1
    nunits = offsets.numel() - 1 if offsets is not None and nlists > 0 else 0
    nsel = sel.numel()
    if units_cap is None and out_offsets is not None:
        units_cap = out_offsets.numel() - 1
    if units_cap is None or out is None:
        nu = nb = 0
        if nsel and nlists > 0 and nunits > 0:
            # the totals of the selections the call will accept; it refuses the others itself
            idx = sel.long() & 0xFFFFFFFF
            ok = idx < nlists
            idx = idx.clamp(max=nlists - 1)
            lu0, lu1 = list_unit[idx].long() & 0xFFFFFFFF, list_unit[idx + 1].long() & 0xFFFFFFFF
            units = (lu1 - lu0).clamp(min=0)
            uf = ufirst.long() & 0xFFFFFFFF if ufirst is not None else torch.zeros_like(units)
            uc = ucount.long() & 0xFFFFFFFF if ufirst is not None else units
            ok = ok & (lu1 <= nunits) & (uf + uc <= units)
            lo = (lu0 + uf).clamp(max=nunits)
            hi = (lo + uc).clamp(max=nunits)
            nu, nb = torch.stack([(uc * ok).sum(), ((offsets[hi] - offsets[lo]).clamp(min=0) * ok).sum()]).tolist()
        if units_cap is None:
            units_cap = int(nu)
        if out is None:
            out = torch.empty(max(int(nb), 1), dtype=torch.uint8, device=dev)[:int(nb)]
    res, res_args = _index_out(dev, nsel, bool(d1) and unit_last is not None, out, out_offsets, units_cap, None, None)
    start0_out = torch.empty(max(nsel, 1), dtype=torch.int32, device=dev)[:nsel] if d1 else None
    L = lib()
    ws = _ws(ws, dev, L.tpf_lists_extract_workspace_size, nsel)
    _check(L.tpf_lists_extract(_ptr(packed), packed.numel() if packed is not None else 0, _ptr(offsets), nunits, _ptr(list_ptr),
                               _ptr(list_unit), nlists, int(bool(d1)), _ptr(start0), _ptr(unit_last), _ptr(sel), _ptr(ufirst), _ptr(ucount),
                               nsel, *res_args[:6], _ptr(start0_out), res_args[6], _ptr(ws), ws.numel(), _ptr(err),
                               stream if stream is not None else _stream(torch)))
    return res[:4] + (start0_out, res[4])
