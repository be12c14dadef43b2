"""CPU tier of the packed-on-device front end (mina_protocol_state_pack_dev, mina_state_frontend_dev, MINA_VERIFY_PACK_ON_DEVICE): the new symbols and the flag are
declared, exported and bound in every layer and refuse bad arguments without a GPU; the new kernels are in the gfx950 code object with nothing in scratch and the
raised wave priority at their top; and the reader itself -- mina_bridge_amd/csrc/state_pack.cuh, the text the kernels are compiled from -- built for the host
(tests/fuzz/state_pack_twin.cpp) agrees with the library's host reader byte for byte on well-formed states, on the exhaustive small mutations of one state, and on
proofs built per chain-selection branch."""
import ctypes
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import code_object as CO  # noqa: E402
import state_pack_helpers as H  # noqa: E402

SYMBOLS = ("mina_protocol_state_pack_dev", "mina_state_frontend_dev")
KERNELS = ("pstate_pack_kernel", "pstate_split_kernel", "pstate_precheck_kernel", "pstate_clear_kernel")
MINA_ERR_ARG = -1


def test_symbols_and_flag_in_every_layer():
    import mina_bridge_amd as m
    hdr = open(os.path.join(ROOT, "include", "mina_verify.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    go = open(os.path.join(ROOT, "bindings", "go", "minaverify.go")).read()
    lib = m.load_library()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, hdr), s
        assert s in m.EXPORTS and hasattr(lib, s), s
        assert "pub fn %s(" % s in rs, s
    assert re.search(r"#define\s+MINA_VERIFY_PACK_ON_DEVICE\s+16u", hdr)
    assert m.lib.VERIFY_PACK_ON_DEVICE == 16
    assert m.lib.VERIFY_PACK_ON_DEVICE & (m.lib.VERIFY_ALLOW_MISSING_KIMCHI | m.lib.VERIFY_ALLOW_UNBOUND_STATEMENT | m.lib.VERIFY_ALLOW_SURROGATE | m.lib.VERIFY_DEDUP_STATES) == 0
    assert "MINA_VERIFY_PACK_ON_DEVICE" in go
    assert "bincode" in hdr[hdr.index("mina_protocol_state_pack_dev") - 3000:hdr.index("mina_protocol_state_pack_dev")]      # the header says why there is no encoding argument
    for meth in ("protocol_state_pack_dev", "state_frontend_dev"):
        assert callable(getattr(m.MinaContext, meth)), meth
    from mina_bridge_amd import build as B
    assert "api_pack.hip" in B.SOURCES and "state_pack.cuh" in B.HEADERS and "consensus.cuh" in B.HEADERS


def test_null_context_is_refused_without_a_gpu():
    import mina_bridge_amd as m
    lib = m.load_library()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n1, z = ctypes.c_size_t(1), ctypes.c_size_t(64)
    assert lib.mina_protocol_state_pack_dev(None, n1, p, z, p, p, p, p, None, p) == MINA_ERR_ARG and lib.mina_last_error()
    assert lib.mina_state_frontend_dev(None, n1, p, z, p, p, p, p, None, p, p, p, None) == MINA_ERR_ARG


needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(CO.LLVM_BIN, "llvm-objdump")), reason="LLVM binutils of the ROCm toolchain not present")


@pytest.fixture(scope="module")
def co():
    c = CO.CodeObjects()
    yield c
    c.close()


@needs_llvm
@pytest.mark.parametrize("kernel", KERNELS)
def test_new_kernels_use_no_scratch_and_raise_their_priority(co, kernel):
    """nothing in scratch BY DESIGN (the reader keeps a state in named registers; tests/test_code_object.py lists every kernel that has scratch, and these are not
    on it), no dynamic stack, no spilled vector register; `s_setprio 2` at the top like every kernel of a job but the chip-filling hashes"""
    ks = co.kernels()
    assert kernel in ks, sorted(k for k in ks if "pstate" in k)
    meta = ks[kernel]
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and not meta.get("uses_dynamic_stack", False), meta
    assert meta["group_segment_fixed_size"] == 0, meta
    ins = co.instructions(kernel)
    assert not any(mn.startswith("scratch_") for _, mn, _ in ins)
    prios = [op.strip() for _, mn, op in ins if mn == "s_setprio"]
    assert prios and set(prios) <= {"2", "0x2"}, prios
    assert "s_setprio" in [mn for _, mn, _ in ins][:40], "the priority is raised at the top of the kernel"


@needs_llvm
def test_pack_kernel_moves_elements_16_bytes_at_a_time(co):
    """the 32-byte field elements go from the wire to the record as 16-byte loads and stores (the blob is read at any alignment), and nothing is staged through LDS"""
    ins = [mn for _, mn, _ in co.instructions("pstate_pack_kernel")]
    assert sum(mn.startswith("global_load_dwordx4") for mn in ins) >= 40 and sum(mn.startswith("global_store_dwordx4") for mn in ins) >= 40
    assert not any(mn.startswith(("ds_read", "ds_write", "ds_load", "ds_store")) for mn in ins)


# ------------------------------------------------------------------------------------------------ the reader's text, compiled for the host
@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or os.path.join(CO.LLVM_BIN, "clang++")
    if not (cxx and os.path.exists(cxx)):
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("state_pack_twin")
    exe = str(d / "state_pack_twin")
    fz = os.path.join(ROOT, "tests", "fuzz")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-w", "-I", os.path.join(fz, "hip_stub"), os.path.join(fz, "state_pack_twin.cpp"), "-o", exe])

    def run(payload: bytes) -> bytes:
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        open(fin, "wb").write(payload)
        subprocess.check_call([exe, fin, fout])
        return open(fout, "rb").read()
    return run


def twin_pack(twin, m, cases, extra=()):
    """mode 0 of the twin over `cases` (+ raw (off, len) entries) -> status, nf, records, infos"""
    blob, off, ln = H.blob_of(cases)
    off = np.concatenate([off, np.array([e[0] for e in extra], np.uint64)]); ln = np.concatenate([ln, np.array([e[1] for e in extra], np.uint32)])
    n = len(off)
    out = twin(struct.pack("<IQ", 0, len(blob)) + blob + struct.pack("<Q", n) + off.tobytes() + ln.tobytes())
    isz = H.info_size(m); per = 1 + 4 + H.REC + isz
    assert len(out) == n * per
    a = np.frombuffer(out, np.uint8).reshape(n, per)
    return a[:, 0], a[:, 1:5].copy().view(np.uint32).reshape(n), a[:, 5:5 + H.REC], a[:, 5 + H.REC:], len(blob)


def test_host_twin_equals_the_host_reader_on_well_formed_states(twin):
    import mina_bridge_amd as m
    cases = [(name, H.bincode_state(st)) for name, st in H.well_formed_states()]
    status, nf, recs, infos, _ = twin_pack(twin, m, cases)
    acc, rej = H.check_pack_results(m, cases, status, nf, recs, infos)
    assert rej == 0 and acc == len(cases) >= 24
    assert {int(x) for x in nf} >= {49}                       # 38 whole + 11 packed elements with 11 sub-windows


def test_host_twin_equals_the_host_reader_on_every_small_mutation(twin):
    import mina_bridge_amd as m
    st = dict(H.well_formed_states())["chain[3]"]
    cases = H.mutations(st)
    blob_probe = H.blob_of(cases)[0]
    past = [(len(blob_probe) - 10, 1542), (len(blob_probe), 1), (len(blob_probe) + 1, 0), ((1 << 64) - 1, 1), ((1 << 64) - 8, 0xffffffff)]      # slices that reach past the blob
    status, nf, recs, infos, blob_len = twin_pack(twin, m, cases, past)
    acc, rej = H.check_pack_results(m, cases, status[:len(cases)], nf, recs, infos)
    print(f"{len(cases)} mutations of one state: {acc} accepted, {rej} rejected by both readers")
    assert acc >= 40 and rej >= 1542                           # every truncation is rejected; `p - 1` in any position and bit flips inside scalars are accepted
    assert not status[len(cases):].any() and not recs[len(cases):].any()


def test_host_twin_precheck_equals_the_host_functions_per_branch(twin):
    import mina_bridge_amd as m
    proofs = H.precheck_proofs()
    blob, begin, end, exp, led, band = H.frontend_inputs(proofs)
    B = len(proofs)
    proofs_past = B                                            # + one range that reaches past the blob
    begin = np.concatenate([begin, np.array([len(blob) - 100], np.uint64)]); end = np.concatenate([end, np.array([len(blob) + 100], np.uint64)])
    exp += bytes(17 * 32); led += bytes(16 * 32); band = np.concatenate([band, np.array([1], np.uint8)])
    out = twin(struct.pack("<IQ", 1, len(blob)) + blob + struct.pack("<Q", B + 1) + begin.tobytes() + end.tobytes() + exp + led + band.tobytes())
    ns = (B + 1) * H.STATES
    assert len(out) == ns * H.REC + ns * 4 + (B + 1) + (B + 1) * 4
    a = np.frombuffer(out, np.uint8)
    recs = a[:ns * H.REC]; nf = a[ns * H.REC:ns * H.REC + 4 * ns].copy().view(np.uint32); pre = a[ns * H.REC + 4 * ns:][:B + 1]; masks = a[ns * H.REC + 4 * ns + B + 1:].copy().view(np.uint32)
    branches = H.check_frontend_results(m, proofs, recs, nf, pre, masks)
    counts = {b: branches.count(b) for b in sorted(set(branches))}
    print(counts)
    for b in H.REQUIRED_BRANCHES:
        assert counts.get(b, 0) >= 1, (b, counts)
    assert masks[proofs_past] == 0 and pre[proofs_past] == 0 and not recs[proofs_past * H.STATES * H.REC:].any()
    assert sum(1 for p, v in zip(proofs, pre) if v) >= 8 and sum(1 for v in pre[:B] if not v) >= 30
