"""The half-precision entry points, without a GPU: they are declared, bound,
and refuse an unknown dtype, an accumulating 2-byte output, any backward
algorithm but STAGED and a misaligned pointer with MAXK_E_ARG before any HIP
call (the child process sees no device, so a missed check would come back as
a positive HIP error, as in test_abi.py's null-buffer sweep)."""
import os
import re
import subprocess
import sys

from spgemm_new_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["maxk_topk_cbsr_t", "maxk_cbsr_scatter_t", "maxk_cbsr_mask_t", "maxk_spgemm_forward_t",
       "maxk_backward_workspace_bytes_t", "maxk_sspmm_backward_t"]


def test_new_entry_points_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(maxk_\w+)\s*\(", text))
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert name in declared, name
    for name, value in (("MAXK_F32", 0), ("MAXK_F16", 1), ("MAXK_BF16", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), text)
        assert getattr(_lib, name) == value
    assert re.search(r"#define MAXK_ABI_VERSION 6\b", text)   # added entry points do not bump it


_CHILD = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
from spgemm_new_amd import _lib
L = ctypes.CDLL(_lib.LIB_PATH)
for name in sys.argv[2:]:
    f = getattr(L, name)
    f.restype, f.argtypes = _lib.SIGNATURES[name]
A = 0x10000            # a non-null, 16-byte aligned dummy address (never dereferenced)
F16, BF16, STAGED = _lib.MAXK_F16, _lib.MAXK_BF16, _lib.MAXK_BWD_STAGED
def topk(x=A, dt=F16, data=A, dense=A):
    return L.maxk_topk_cbsr_t(x, dt, 8, 256, 256, 32, 0, data, A, dense, None)
def scatter(f, vals=A, dt=F16, out=A):
    return f(vals, dt, A, 8, 32, 256, out, None)
def fwd(data=A, ddt=F16, flags=0, out=A, odt=F16, parts=None, ws=A):
    return L.maxk_spgemm_forward_t(A, 4, A, A, A, data, ddt, A, 8, 256, 32, flags, parts, 0, out,
                                   odt, ws, 1 << 30, None)
def bwd(algo=STAGED, grad=A, gdt=F16, dxs=A, xdt=F16, ws=A):
    return L.maxk_sspmm_backward_t(algo, A, 4, A, A, A, grad, gdt, A, 8, 8, 64, 256, 32, dxs, xdt,
                                   A, A, 4, A, ws, 1 << 30, None)
cases = {
    "topk dtype 3": topk(dt=3),
    "scatter dtype 3": scatter(L.maxk_cbsr_scatter_t, dt=3),
    "mask dtype 3": scatter(L.maxk_cbsr_mask_t, dt=3),
    "forward data dtype 3": fwd(ddt=3),
    "forward out dtype 3": fwd(odt=3),
    "backward grad dtype 3": bwd(gdt=3),
    "backward dxs dtype 3": bwd(xdt=3),
    "forward accumulate f16 out": fwd(flags=_lib.MAXK_FWD_ACCUMULATE),
    "forward accumulate bf16 out": fwd(ddt=BF16, odt=BF16, flags=_lib.MAXK_FWD_ACCUMULATE),
    "forward accumulate f32 data bf16 out": fwd(ddt=_lib.MAXK_F32, odt=BF16,
                                                 flags=_lib.MAXK_FWD_ACCUMULATE),
    "topk misaligned x": topk(x=A + 2),
    "topk misaligned data": topk(data=A + 2),
    "topk misaligned dense": topk(dense=A + 2),
    "scatter misaligned out": scatter(L.maxk_cbsr_scatter_t, out=A + 2),
    "mask misaligned src": scatter(L.maxk_cbsr_mask_t, vals=A + 2),
    "forward misaligned data": fwd(data=A + 2),
    "forward misaligned out": fwd(out=A + 2),
    "forward misaligned parts": fwd(parts=A + 2),
    "backward misaligned grad": bwd(grad=A + 2),
    "backward misaligned dxs": bwd(dxs=A + 2),
}
for algo in ("ATOMIC", "LOCAL", "TILE", "STAGED_EDGE", "EDGE_GATHER", "APPEND"):
    cases["backward f16 " + algo] = bwd(algo=getattr(_lib, "MAXK_BWD_" + algo))
    cases["backward bf16 " + algo] = bwd(algo=getattr(_lib, "MAXK_BWD_" + algo), gdt=BF16, xdt=BF16)
cases["backward f32 grad f16 dxs ATOMIC"] = bwd(algo=_lib.MAXK_BWD_ATOMIC, gdt=_lib.MAXK_F32)
for what, rc in cases.items():
    print(f"{rc}\t{what}", flush=True)
"""


def test_bad_dtype_flags_algo_and_alignment_return_e_arg():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, *NEW], capture_output=True, text=True,
                       timeout=300, env=env)
    lines = p.stdout.strip().splitlines()
    assert p.returncode == 0, (lines[-1:], p.stderr[-2000:])
    assert len(lines) >= 30
    for ln in lines:
        rc, what = ln.split("\t")
        assert int(rc) == _lib.MAXK_E_ARG, f"{what}: returned {rc}, expected MAXK_E_ARG"


def test_backward_workspace_of_a_half_dxs_has_the_owner_rows():
    L = _lib.load()
    E, k, CP = 1000, 32, 7
    base = L.maxk_backward_workspace_bytes(_lib.MAXK_BWD_STAGED, E, k, CP)
    assert L.maxk_backward_workspace_bytes_t(_lib.MAXK_BWD_STAGED, E, k, CP, _lib.MAXK_F32) == base
    for dt in (_lib.MAXK_F16, _lib.MAXK_BF16):
        n = L.maxk_backward_workspace_bytes_t(_lib.MAXK_BWD_STAGED, E, k, CP, dt)
        assert base + CP * k * 4 <= n <= base + CP * k * 4 + 256


def test_training_example_lists_amp():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_maxk_sage.py"),
                        "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--amp" in p.stdout and "bf16" in p.stdout and "fp16" in p.stdout
