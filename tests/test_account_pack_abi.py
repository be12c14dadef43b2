"""CPU tier of the device path of Proof-of-Account (mina_account_frontend_dev, mina_account_job_dev, MINA_VERIFY_ACCOUNT_ON_DEVICE): the new symbols and the flag are
declared, exported and bound in every layer and refuse bad arguments without a GPU; the new kernels are in the gfx950 code object with nothing in scratch, no LDS and
the raised wave priority at their top; and the reader itself -- mina_bridge_amd/csrc/account_pack.cuh, the text the kernels are compiled from -- built for the host
(tests/fuzz/account_pack_twin.cpp) agrees with the oracle's `to_input` fields on well-formed pairs and with the library's host readers on every truncation and every
byte position of one full zkApp proof."""
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
import account_pack_helpers as H  # noqa: E402

SYMBOLS = ("mina_account_frontend_dev", "mina_account_job_dev")
KERNELS = ("acct_frontend_kernel", "acct_verdict_kernel", "acct_hash_kernel<0, 16>", "acct_hash_kernel<0, 8>", "acct_hash_kernel<0, 3>", "acct_fold_kernel<0, 16>",
           "acct_fold_kernel<0, 8>", "acct_fold_kernel<0, 3>")
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
    assert re.search(r"#define\s+MINA_VERIFY_ACCOUNT_ON_DEVICE\s+32u", hdr)
    L = m.lib
    assert L.VERIFY_ACCOUNT_ON_DEVICE == 32
    assert L.VERIFY_ACCOUNT_ON_DEVICE & (L.VERIFY_ALLOW_MISSING_KIMCHI | L.VERIFY_ALLOW_UNBOUND_STATEMENT | L.VERIFY_ALLOW_SURROGATE | L.VERIFY_DEDUP_STATES | L.VERIFY_PACK_ON_DEVICE) == 0
    assert "MINA_VERIFY_ACCOUNT_ON_DEVICE" in go
    assert "bincode" in hdr[hdr.index("mina_account_frontend_dev") - 3000:hdr.index("mina_account_frontend_dev")]      # the header says why there is no encoding argument
    for meth in ("account_frontend_dev", "account_job_dev"):
        assert callable(getattr(m.MinaContext, meth)), meth
    from mina_bridge_amd import build as B
    assert "api_account_dev.hip" in B.SOURCES and {"account_pack.cuh", "pack_common.cuh", "state_pack.cuh"} <= set(B.HEADERS)


def test_null_context_is_refused_without_a_gpu():
    import mina_bridge_amd as m
    lib = m.load_library()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n1, z = ctypes.c_size_t(1), ctypes.c_size_t(64)
    assert lib.mina_account_frontend_dev(None, n1, p, z, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p) == MINA_ERR_ARG and lib.mina_last_error()
    assert lib.mina_account_job_dev(None, n1, p, z, p, p, p, p, p, p, None, None) == MINA_ERR_ARG


needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(CO.LLVM_BIN, "llvm-objdump")), reason="LLVM binutils of the ROCm toolchain not present")


@pytest.fixture(scope="module")
def co():
    c = CO.CodeObjects()
    yield c
    c.close()


@needs_llvm
@pytest.mark.parametrize("kernel", KERNELS)
def test_new_kernels_use_no_scratch_and_raise_their_priority(co, kernel):
    """nothing in scratch BY DESIGN (tests/test_code_object.py lists every kernel that has scratch, and these are not on it), no dynamic stack, no spilled vector
    register, no LDS; `s_setprio 2` at the top like every kernel of a job but the chip-filling hashes"""
    ks = co.kernels()
    assert kernel in ks, sorted(k for k in ks if "acct" in k)
    meta = ks[kernel]
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and not meta.get("uses_dynamic_stack", False), meta
    assert meta["group_segment_fixed_size"] == 0, meta
    ins = co.instructions(kernel)
    assert not any(mn.startswith("scratch_") for _, mn, _ in ins)
    assert not any(mn.startswith(("ds_read", "ds_write", "ds_load", "ds_store")) for _, mn, _ in ins)
    prios = [op.strip() for _, mn, op in ins if mn == "s_setprio"]
    assert prios and set(prios) <= {"2", "0x2"}, prios
    assert "s_setprio" in [mn for _, mn, _ in ins][:40], "the priority is raised at the top of the kernel"


@needs_llvm
def test_front_end_moves_elements_16_bytes_at_a_time(co):
    """the field elements go from the wire to their record slot as 16-byte stores, and the compacted list is taken with one atomic add"""
    ins = [mn for _, mn, _ in co.instructions("acct_frontend_kernel")]
    assert sum(mn.startswith("global_store_dwordx4") for mn in ins) >= 20
    assert sum(mn.startswith("global_atomic_add") for mn in ins) == 1


# ------------------------------------------------------------------------------------------------ the reader's text, compiled for the host
@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or os.path.join(CO.LLVM_BIN, "clang++")
    if not (cxx and os.path.exists(cxx)):
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("account_pack_twin")
    exe = str(d / "account_pack_twin")
    fz = os.path.join(ROOT, "tests", "fuzz")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-w", "-I", os.path.join(fz, "hip_stub"), os.path.join(fz, "account_pack_twin.cpp"), "-o", exe])

    def run(pairs, roots):
        """pairs [(proof, pub)], roots n x 32 bytes -> (front-end outputs, passed, ran)"""
        blob, po, pl, qo, ql = H.blob_of(pairs)
        n = len(pairs)
        extra = [(len(blob) - 5, 100, 3, 40), ((1 << 64) - 1, 1, 3, 40), (3, 40, len(blob) + 1, 0), ((1 << 64) - 8, (1 << 64) - 1, (1 << 64) - 40, 41)]      # slices that reach past the blob
        po, pl, qo, ql = (np.concatenate([x, np.array([e[j] for e in extra], np.uint64)]) for j, x in enumerate((po, pl, qo, ql)))
        nn = n + len(extra)
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        with open(fin, "wb") as fh:
            fh.write(struct.pack("<Q", len(blob)) + blob + struct.pack("<Q", nn) + po.tobytes() + pl.tobytes() + qo.tobytes() + ql.tobytes() + bytes(roots) + bytes(32 * len(extra)))
        subprocess.check_call([exe, fin, fout])
        out = open(fout, "rb").read()
        raw, at = {}, 0
        for name, size in H.FRONTEND_SIZES:
            raw[name] = out[at:at + size(nn)]; at += size(nn)
        passed = np.frombuffer(out[at:at + 4 * nn], np.uint32); ran = np.frombuffer(out[at + 4 * nn:at + 8 * nn], np.uint32)
        assert at + 8 * nn == len(out)
        f = H.unpack_frontend(raw, nn)
        assert not (f["bits"][n:] & H.CHECK_FORMAT).any() and not f["nfields"].reshape(4, nn)[:, n:].any() and (passed[n:] == 0).all() and (ran[n:] == H.CHECK_FORMAT).all(), "a slice past the blob is rejected"
        # stage s of entry k sits at [s * nn + k]: re-index for the n real pairs
        f["records"] = f["records"].reshape(4, nn, H.REC)[:, :n].reshape(4 * n, H.REC)
        for k in ("nfields", "salt_idx"): f[k] = f[k].reshape(4, nn)[:, :n].reshape(-1)
        for k in ("siblings", "dirs", "depths", "ledger", "marks", "bits"): f[k] = f[k][:n]
        return f, passed[:n], ran[:n]
    return run


def verdict_rule(f, roots, i):
    b = int(f["bits"][i])
    if not b & H.CHECK_FORMAT:
        return 0, H.CHECK_FORMAT
    same = bytes(roots[32 * i:32 * i + 32]) == f["ledger"][i].tobytes()
    return H.CHECK_FORMAT | (b & H.CHECK_ACCOUNT_ABI) | (H.CHECK_MERKLE if same else 0), H.CHECK_FORMAT | H.CHECK_ACCOUNT_ABI | H.CHECK_MERKLE


def test_host_twin_equals_the_oracle_on_well_formed_pairs(twin):
    import mina_bridge_amd as m
    from ipa_helpers import poseidon_pp
    cases = H.well_formed_pairs()
    roots = b"".join(c[2][:32] if i % 2 == 0 else bytes(32) for i, c in enumerate(cases))      # every other pair: the root the fold would have to produce
    f, passed, ran = twin([(c[1], c[2]) for c in cases], roots)
    n = len(cases)
    refs, classes = H.check_frontend(m, [(c[0], c[1], c[2]) for c in cases], f)
    assert classes == ["abi passes"] * n and n >= 24
    H.check_records(cases, f, poseidon_pp(0))
    assert f["zk_count"] == sum(1 for c in cases if c[3]["zkapp"] is not None) == 16
    for i, c in enumerate(cases):
        assert int(f["depths"][i]) == len(c[4]) and (int(passed[i]), int(ran[i])) == verdict_rule(f, roots, i) == ((1 | 64 | 128) if i % 2 == 0 else (1 | 64), 1 | 64 | 128), c[0]


def test_host_twin_equals_the_host_readers_on_every_truncation_and_byte(twin):
    """one full zkApp proof (key, timing, delegate, symbol, a 31-byte URI, depth 2): every truncation, a trailing byte, every byte position with several replacement
    values, against mina_parse_merkle_path, mina_parse_account_pub_inputs and mina_account_abi_encode(.., MINA_ENC_BINCODE); the same sweep over the public input"""
    import random
    import mina_bridge_amd as m
    from oracle import mina_account_ref as A
    rng = random.Random(H.SEED + 7)
    a = A.synth_account(rng, True, True, True, with_vk=True)
    a["token_symbol"] = b"SWEEP!"; a["zkapp"]["zkapp_uri"] = bytes(rng.randrange(256) for _ in range(31))
    path = H.random_path(rng, 2)
    proof, pub = A.write_account_proof(path, a), H.pub_input(rng.randrange(H.P), A.abi_encode_account(a))
    for what, muts, pair in (("proof", H.proof_mutations(proof), lambda b: (b, pub)), ("public input", H.proof_mutations(pub), lambda b: (proof, b))):
        pairs = [pair(b) for _, b in muts]
        roots = b"".join(q[:32].ljust(32, b"\0") if i % 2 == 0 else bytes(32) for i, (_, q) in enumerate(pairs))
        f, passed, ran = twin(pairs, roots)
        refs, classes = H.check_frontend(m, [(name, p, q) for (name, _), (p, q) in zip(muts, pairs)], f)
        counts = {c: classes.count(c) for c in sorted(set(classes))}
        print(what, len(pairs), "cases:", counts)
        assert counts.get("format fails", 0) >= len(muts[0][1]) and counts.get("abi fails", 0) >= 100 and counts.get("abi passes", 0) >= 1, counts
        for i in range(len(pairs)):
            assert (int(passed[i]), int(ran[i])) == verdict_rule(f, roots, i), muts[i][0]
