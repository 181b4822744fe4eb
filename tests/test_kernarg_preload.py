"""The built step kernels receive their launch scalars and first pointers in preloaded SGPRs (CPU only, on
the objects the library was linked from): for every translation unit on build.py's preload list each step
kernel's descriptor asks for a kernel-argument preload, and the main entry of each by-value kernel -- past
the 256-byte compatibility prologue -- reaches the first state load without waiting for a scalar load.
Also: every object was built at code-generation gate variant 0 (no fallback ships)."""
import glob
import importlib.util
import os
import re
import struct
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
OBJDIR = os.path.join(ROOT, "gym-futbol_amd", "build", "obj")
LLVM = "/opt/rocm/lib/llvm/bin"
STEP = re.compile(r"v1_step_kernel|v0_step_kernel|v0_rollout_kernel")
# the kernels that take the launch scalars by value: futbol::by_value::v1_step_kernel<N, 64, OT, DEF>,
# futbol::v0_step_kernel<OT> -- and of those the registered ids' (DEF = true: the default field)
BYVAL = re.compile(r"by_value14v1_step_kernelILi\d+ELi64E[fd]Lb[01]EE|v0_step_kernelI[fd]EE")
HOT = re.compile(r"by_value14v1_step_kernelILi\d+ELi64E[fd]Lb1EE|v0_step_kernelI[fd]EE")
built = pytest.mark.skipif(not glob.glob(os.path.join(OBJDIR, "futbol_*.hip.o")) or
                           not os.path.exists(LLVM + "/llvm-objdump"), reason="no built objects / ROCm LLVM tools")


def _preload_objects():
    """the objects of build.py's preload list (the project's build.py by path: `import build` could be
    another installed module); skips when the library was built without the option (FUTBOL_PRELOAD=0)"""
    spec = importlib.util.spec_from_file_location("futbol_build", os.path.join(ROOT, "gym-futbol_amd", "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    if B.PRELOAD in ("", "0"):
        pytest.skip("built with FUTBOL_PRELOAD=0")
    assert B.PRELOAD_SOURCES, "the preload list is empty"
    return [os.path.join(OBJDIR, s + ".o") for s in sorted(B.PRELOAD_SOURCES)]


def _descriptors(co):
    """{kernel: its 64-byte kernel descriptor} of an AMDGPU code object (the <kernel>.kd objects)"""
    secs, syms = {}, []
    out = subprocess.run([LLVM + "/llvm-readelf", "-S", "-s", "-W", co], capture_output=True, text=True, check=True).stdout
    for ln in out.splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", ln)
        if m:
            secs[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))  # address, file offset
        m = re.match(r"\s*\d+:\s+([0-9a-f]+)\s+64\s+OBJECT\s+\S+\s+\S+\s+(\d+)\s+(\S+)\.kd$", ln)
        if m:
            syms.append((m.group(3), int(m.group(1), 16), int(m.group(2))))
    raw = open(co, "rb").read()
    kd = {}
    for name, addr, sec in syms:
        a, off = secs[sec]
        kd[name] = raw[off + addr - a:off + addr - a + 64]
    return kd


@built
def test_step_kernels_ask_for_a_kernarg_preload():
    import isa_exec_check as I
    for o in _preload_objects():
        with tempfile.TemporaryDirectory(prefix="kd_") as tmp:
            (co,) = I.code_objects(o, tmp)
            kd = _descriptors(co)
        steps = {k: d for k, d in kd.items() if STEP.search(k)}
        assert len(steps) == (4 if "_v0" in o else 8), (o, sorted(kd))  # {f32, f64} x {step, rollout} (x geometry)
        assert sum(1 for k in steps if BYVAL.search(k)) == len(steps) // 2, sorted(steps)  # the single steps
        for k, d in steps.items():
            # kernel descriptor bytes 58-59: KERNARG_PRELOAD_SPEC_LENGTH (bits 0-6, dwords), _OFFSET (bits 7-15)
            (spec,) = struct.unpack_from("<H", d, 58)
            # by value: all 14 leading dwords; the rollouts (params pointer first, then a struct): the pointer
            want = 14 if BYVAL.search(k) else 2
            assert spec & 0x7F == want, "%s %s: preload length %d" % (os.path.basename(o), k[:70], spec & 0x7F)


@built
def test_main_entry_reaches_the_first_state_load_without_a_scalar_wait():
    """The entry the hardware uses when it preloads is the kernel's address + 256 (the prologue before it,
    s_load + s_waitcnt + s_branch padded with s_nop, is for firmware without the feature); every step and
    rollout kernel of a listed TU has that shape.  From the main entry of a by-value kernel of the
    registered ids (the default field) to its first global load into registers -- the state; v0's LDS-DMA
    loads of the pow tables (global_load_lds, pc-relative addresses) come before it, inside the checked
    window -- nothing waits on lgkmcnt (the scalar load of the later arguments may be issued there).  Not
    checked for the runtime-geometry instances, which fetch the segment table through the params pointer
    first (it is not among the 14 preloaded dwords), nor for the rollouts, which read B through it."""
    import isa_exec_check as I
    import isa_liveness as L
    hot = 0
    objs = _preload_objects()
    for o in objs:
        for dis in I.disassemble(o):
            for k, ins in L.parse(dis).items():
                if not STEP.search(k):
                    continue
                base = ins[0][0]
                head = [t for a, t in ins if a < base + 256]
                assert head[0].startswith("s_load_dword") and any(t.startswith("s_branch") for t in head), k
                assert all(t.startswith(("s_load_dword", "s_waitcnt", "s_branch", "s_nop")) for t in head), k
                if not HOT.search(k):
                    continue
                hot += 1
                main = [t for a, t in ins if a >= base + 256]
                first = next(i for i, t in enumerate(main) if re.match(r"global_load_dword", t))
                waits = [t for t in main[:first] if t.startswith("s_waitcnt") and "lgkmcnt" in t]
                assert not waits, "%s %s: %s" % (os.path.basename(o), k[:70], waits)
    assert hot == 2 * len(objs)  # f32 and f64 outputs of every listed TU


@built
def test_every_object_is_built_at_gate_variant_0():
    stamps = sorted(glob.glob(os.path.join(OBJDIR, "*.cmd")))
    assert len(stamps) == len(glob.glob(os.path.join(ROOT, "gym-futbol_amd", "csrc", "*.hip")))
    for s in stamps:
        txt = open(s).read()
        assert "\n#gate variant 0: default" in txt, "%s: %s" % (os.path.basename(s), txt[txt.find("#gate"):][:200])

