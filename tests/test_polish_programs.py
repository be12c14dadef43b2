"""PolishToken programs on the CPU: the validator and the host interpreter of mina_bridge_amd/csrc/polish.h (compiled into the stand-alone program
tests/fuzz/polish_twin.cpp, plainly and under AddressSanitizer + UBSan) against tests/polish_model.py, on the generated program families under all 256
feature-flag combinations and both fields, and on a mutation sweep of their byte-code.  No GPU; nothing is loaded into the interpreter."""
import os
import random
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import fe32_model as M
import polish_model as PM
from oracle import kimchi_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20
ALL_FLAGS = [[bool(i >> j & 1) for j in range(8)] for i in range(256)]
FEATURE_MASKS = [K.feature_mask(f) for f in ALL_FLAGS]
ALL_PRESENT = (1 << PM.N_SLOTS) - 1
# the programs the mutation sweep starts from.  Of a natural program's opcode substitutions about one in eight decodes (a binary operator has two stand-ins, a push
# with operands next to none), so beside the short programs of the families stand two-token ones written for the sweep: a push and a POW whose exponent bytes are
# themselves opcodes, `ADD (DUP MUL)* STORE`.  A push put in place of that POW leaves a program the validator has to follow to its end, and which then runs.
N_SWEEP = 132
SWEEP_SEEDS = ("deep/stack24", "deep/cache8", "regions/nest3", "regions/length1", "regions/ends_on_last_token", "regions/nested_end_on_last_token",
               "regions/back_to_back", "regions/stores", "bad_load/feature6") + tuple("sweep/%d" % i for i in range(N_SWEEP))


def make_env(side, seed, log2_domain, zk_rows):
    _, r, ncols = PM.SIDES[side]
    rng = random.Random("env/%s/%d" % (side, seed))
    f = lambda: rng.randrange(r)
    return PM.Env(r, log2_domain, zk_rows, f(), f(), f(), f(), f(), f(), [[f() for _ in range(3)] for _ in range(3)], [(f(), f()) for _ in range(ncols)],
                  present=None if side == PM.WRAP else ALL_PRESENT)


def sweep_programs(side):
    rng = random.Random("sweep/" + side)
    binop = lambda: rng.choice([K.T_ADD, K.T_MUL, K.T_SUB])
    pw = lambda: (K.T_POW, int.from_bytes(bytes([binop(), K.T_DUP, binop(), K.T_DUP, binop(), K.T_DUP, binop(), K.T_STORE]), "little"))
    pushes = [(K.T_ALPHA,), (K.T_BETA,), (K.T_GAMMA,), (K.T_JOINT,), (K.T_ENDO,), (K.T_VANISH_ZK,)]
    out = []
    while len(out) < N_SWEEP:                                      # every push in front of the same POW: a substituted push is then another seed, run once
        p = pw()
        out += [PM.Program("sweep/%d" % (len(out) + j), [x, p], True) for j, x in enumerate(pushes)]
    return out


@pytest.fixture(scope="module")
def families():
    return {side: PM.programs(side, SEED) + sweep_programs(side) for side in (PM.WRAP, PM.STEP)}


# ------------------------------------------------------------------------------------------------ the twin
def _cxx():
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not (cxx and os.path.exists(cxx)):
        pytest.skip("no C++ compiler")
    return cxx


def _build(d, extra, name):
    fz = os.path.join(ROOT, "tests", "fuzz")
    exe = str(d / name)
    done = subprocess.run([_cxx(), "-std=c++17", "-O1", "-w", *extra, "-I", os.path.join(fz, "hip_stub"), os.path.join(fz, "polish_twin.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, done


@pytest.fixture(scope="module")
def twin_plain(tmp_path_factory):
    exe, done = _build(tmp_path_factory.mktemp("polish_twin"), [], "polish_twin")
    assert done.returncode == 0, done.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def twin_asan(tmp_path_factory):
    """a stand-alone program with its own main"""
    exe, done = _build(tmp_path_factory.mktemp("polish_twin_asan"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "polish_twin_asan")
    if done.returncode != 0:
        assert re.search(r"asan|ubsan|sanitize", done.stderr, re.I), done.stderr[-4000:]
        pytest.skip("the compiler has no AddressSanitizer / UBSan runtime")
    return exe


def section(side, env, code, masks, reuse=False):
    field, r, ncols = PM.SIDES[side]
    if reuse:                                                      # the environment and the masks of the section before it
        return struct.pack("<8I", field | 0x100, ncols, env.log2_domain, env.zk_rows, 0 if env.present is None else 1, len(env.evals), len(code), len(masks)) + code + bytes(-len(code) % 4)
    zkpm, zeta_n = env.vanishes_on_zk_rows(), pow(env.zeta, 1 << env.log2_domain, r)
    vals = [env.alpha, env.beta, env.gamma, env.endo, zkpm, env.zeta, zeta_n, env.omega, env.joint] + [x for row in env.mds for x in row] + [x for pair in env.evals for x in pair]
    out = struct.pack("<8I", field, ncols, env.log2_domain, env.zk_rows, 0 if env.present is None else 1, len(env.evals), len(code), len(masks))
    out += np.array([M.words(c) for c in M.field(field).consts], np.uint32).tobytes()
    out += b"".join(int(v).to_bytes(32, "little") for v in vals)
    out += code + bytes(-len(code) % 4)
    out += b"".join(struct.pack("<2I", f, p) for f, p in masks)
    return out


def run_twin(exe, d, sections):
    """sections: [(side, env, code, masks)] -> [None where the validator refused, else [(verdict, value)] per mask]; the program must end with a clean exit"""
    fin, fout = str(d / "in.bin"), str(d / "out.bin")
    with open(fin, "wb") as fh:
        for i, s in enumerate(sections):
            fh.write(section(*s, reuse=i > 0 and s[1] is sections[i - 1][1] and s[3] is sections[i - 1][3]))
    done = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-6000:])
    raw = np.fromfile(fout, np.uint32)
    at, res = 0, []
    for _, _, _, masks in sections:
        acc = int(raw[at]); at += 1
        if not acc:
            res.append(None)
            continue
        rows = raw[at:at + 9 * len(masks)].reshape(len(masks), 9); at += 9 * len(masks)
        res.append([(int(row[0]), int.from_bytes(row[1:].tobytes(), "little")) for row in rows])
    assert at == raw.size
    return res


def model_rows(tokens, env, masks):
    """[(verdict, value)] of the model per (feature mask, presence mask): evaluated once for every distinct outcome of the feature codes the program looks at"""
    used, memo, out = PM.features_used(tokens), {}, []
    for f, p in masks:
        key = (tuple(f >> c & 1 for c in used), p)
        if key not in memo:
            try:
                memo[key] = (1, PM.evaluate(tokens, env.with_masks(f, None if env.present is None else p)))
            except LookupError:
                memo[key] = (0, 0)
        out.append(memo[key])
    return out


def masks_of(side):
    m = [(f, 0 if side == PM.WRAP else ALL_PRESENT) for f in FEATURE_MASKS]
    if side == PM.STEP:                                            # and proofs that do not carry every optional evaluation
        rng = random.Random(5)
        m += [(FEATURE_MASKS[255], p) for p in (0, 1, ALL_PRESENT ^ 1, ALL_PRESENT >> 1)] + [(FEATURE_MASKS[rng.randrange(256)], rng.getrandbits(PM.N_SLOTS)) for _ in range(12)]
    return m


ENVS = {PM.WRAP: [(6, 3), (6, 8), (15, 1)], PM.STEP: [(10, 3), (16, 8), (13, 5)]}         # (log2 domain, zk_rows)


# ------------------------------------------------------------------------------------------------ tests
def test_the_generator_is_deterministic_and_covers_what_it_says(families):
    for side in (PM.WRAP, PM.STEP):
        _, r, ncols = PM.SIDES[side]
        progs = families[side]
        again = PM.programs(side, SEED)
        assert [(p.name, p.tokens) for p in again] == [(p.name, p.tokens) for p in progs[:len(again)]]
        assert len({p.name for p in progs}) == len(progs)
        fams = {p.name.split("/")[0] for p in progs}
        assert {"all_ops", "deep", "pow", "lagrange", "regions", "bad_load", "long", "random"} <= fams
        toks = [t for p in progs if p.valid for t in p.tokens]
        assert {t[0] for t in toks} == set(range(19))
        assert {(t[1], t[2]) for t in toks if t[0] == K.T_MDS} == {(i, j) for i in range(3) for j in range(3)}
        assert {(t[1], t[2]) for t in toks if t[0] == K.T_CELL} == {(c, row) for c in range(ncols) for row in (0, 1)}
        assert {0, 1, r - 1} <= {t[1] for t in toks if t[0] == K.T_LITERAL}
        assert {0, 1, 2, 7, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - 1} <= {t[1] for t in toks if t[0] == K.T_POW}
        n = 1 << ENVS[side][0][0]
        assert {0, 1, n - 1, n, -1, -2, PM.INT32_MIN} <= {t[1] for t in toks if t[0] == K.T_LAGRANGE}
        assert {t[1] for t in toks if t[0] in (K.T_SKIP_IF, K.T_SKIP_IF_NOT)} == set(range(PM.N_FEATURES))
        by = {p.name: p for p in progs}
        assert 2000 <= len(by["long/chain"].tokens) <= 6000 and sum(p.name.startswith("random/") for p in progs) == 12

        def peaks(tokens):            # deepest stack and fullest cache over all feature masks, on a shadow of the model's loop
            deep = full = 0
            for f in set(tuple(m >> c & 1 for c in PM.features_used(tokens)) for m in FEATURE_MASKS):
                on = dict(zip(PM.features_used(tokens), f)); d = c = skip = 0
                for t in tokens:
                    if skip: skip -= 1; continue
                    if t[0] in (K.T_SKIP_IF, K.T_SKIP_IF_NOT):
                        if bool(on[t[1]]) == (t[0] == K.T_SKIP_IF): skip = t[2]; d += 1
                    elif t[0] in PM.PUSHES: d += 1
                    elif t[0] in (K.T_ADD, K.T_MUL, K.T_SUB): d -= 1
                    elif t[0] == K.T_STORE: c += 1
                    deep, full = max(deep, d), max(full, c)
            return deep, full
        assert peaks(by["deep/stack24"].tokens)[0] == 24 and peaks(by["deep/cache8"].tokens)[1] == 8 and peaks(by["deep/both"].tokens) == (24, 8)
        assert {t[1] for t in by["deep/cache8"].tokens if t[0] == K.T_LOAD} == set(range(8))
        assert peaks(by["deep/stack25"].tokens)[0] == 25 and peaks(by["deep/cache9"].tokens)[1] == 9
        # the validator's restatement accepts exactly the ones marked valid, and the named refusals are refused
        for p in progs:
            assert (PM.decode(PM.encode(p.tokens), r, ncols) is not None) == p.valid, p.name
            if p.valid: assert PM.decode(PM.encode(p.tokens), r, ncols) == [tuple(t) for t in p.tokens], p.name
        assert all(PM.decode(code, r, ncols) is None for code in PM.refusals(side).values())
        assert PM.decode(b"", r, ncols) == []


def test_the_encoder_refuses_operands_that_do_not_fit():
    from kimchi_helpers import encode_tokens
    for bad in ([(K.T_POW, 1 << 64)], [(K.T_POW, -1)], [(K.T_LAGRANGE, 1 << 31)], [(K.T_LAGRANGE, -(1 << 31) - 1)]):
        with pytest.raises(ValueError):
            encode_tokens([(K.T_ALPHA,)] + bad)
    assert encode_tokens([(K.T_POW, (1 << 64) - 1), (K.T_LAGRANGE, -(1 << 31))]) == bytes([K.T_POW]) + b"\xff" * 8 + bytes([K.T_LAGRANGE]) + b"\x00\x00\x00\x80"


def test_the_model_and_the_oracle_interpreter_agree_on_every_program_and_mask(families):
    """oracle/kimchi_ref.py polish_evaluate is the GPU tests' second checker: pinned here to the model, which is written without it"""
    for side in (PM.WRAP, PM.STEP):
        _, r, _ = PM.SIDES[side]
        masks = masks_of(side)
        for log2, zk in ENVS[side][:1]:
            env = make_env(side, 2, log2, zk)
            index = type("Ix", (), {"n": 1 << log2, "log2_domain": log2, "zk_rows": zk})()
            for p in families[side]:
                if not p.valid: continue
                want = cached_rows(side, 2, log2, zk, p, masks)
                used, memo = PM.features_used(p.tokens), {}
                for (f, pm), w in zip(masks, want):
                    key = (tuple(f >> c & 1 for c in used), pm)
                    if key not in memo:
                        consts = {"alpha": env.alpha, "beta": env.beta, "gamma": env.gamma, "joint_combiner": env.joint, "endo": env.endo, "mds": env.mds, "features": f,
                                  "present": None if side == PM.WRAP else pm}
                        try:
                            memo[key] = (1, K.polish_evaluate(p.tokens, index, env.zeta, env.evals, consts, r))
                        except KeyError:
                            memo[key] = (0, 0)
                    assert memo[key] == w, (side, p.name, f, pm)
                if p.name.startswith("bad_load"):
                    assert [v for v, _ in want[:256]] == [f >> 6 & 1 for f in FEATURE_MASKS]


_ROWS = {}


def cached_rows(side, seed, log2, zk, p, masks):
    """the model's rows of a generated program in the environment make_env(side, seed, log2, zk): computed once for the tests of this file"""
    key = (side, seed, log2, zk, p.name)
    if key not in _ROWS:
        _ROWS[key] = model_rows(p.tokens, make_env(side, seed, log2, zk), masks)
    return _ROWS[key]


def check_families(exe, d, families):
    secs, wants, names = [], [], []
    for side in (PM.WRAP, PM.STEP):
        masks = masks_of(side)
        for i, (log2, zk) in enumerate(ENVS[side]):
            env = make_env(side, 2 + i, log2, zk)
            for p in families[side]:
                if i and p.name.split("/")[0] not in ("lagrange", "regions", "all_ops", "bad_load"): continue        # the other domains / zk_rows: where they matter
                secs.append((side, env, PM.encode(p.tokens), masks)); names.append((side, p.name, log2, zk))
                wants.append(cached_rows(side, 2 + i, log2, zk, p, masks) if p.valid else None)
        secs.append((side, make_env(side, 9, ENVS[side][0][0], 3), b"", masks[:2])); names.append((side, "empty", 0, 0)); wants.append("empty")
        for name, code in PM.refusals(side).items():
            secs.append((side, make_env(side, 9, ENVS[side][0][0], 3), code, masks[:2])); names.append((side, name, 0, 0)); wants.append(None)
    got = run_twin(exe, d, secs)
    for g, w, n in zip(got, wants, names):
        if w == "empty":
            assert g is not None and all(v == 0 for v, _ in g), n          # accepted by the validator; the interpreter leaves no value and says so (the callers do not run it)
        else:
            assert g == w, (n, "accepted" if g is not None else "refused", [i for i in range(len(w or []))if g and g[i] != w[i]][:8])
    return len(secs)


def test_every_family_under_all_flag_combinations_both_fields(twin_plain, tmp_path, families):
    assert check_families(twin_plain, tmp_path, families) > 80


def test_every_family_under_the_address_and_undefined_behaviour_sanitizers(twin_asan, tmp_path, families):
    check_families(twin_asan, tmp_path, families)


def test_mutation_sweep_accepts_and_refuses_with_the_model_and_stays_in_bounds(twin_asan, tmp_path, families):
    """every truncation, every opcode substitution and the operand edges of the seed programs: the validator and its restatement accept the same mutants, and an
    accepted one runs under all 256 masks in the sanitized build -- a clean exit (stack[24] and cache[8] in bounds) and the model's verdicts and values"""
    secs, wants, kinds, subs = [], [], [], []
    for side in (PM.WRAP, PM.STEP):
        _, r, ncols = PM.SIDES[side]
        masks = masks_of(side)[:256]
        env = make_env(side, 3, ENVS[side][0][0], 3)
        by = {p.name: p for p in families[side]}
        seen = set()
        for name in SWEEP_SEEDS:
            for kind, code in PM.mutants(by[name].tokens, r, ncols):
                toks = PM.decode(code, r, ncols)
                if kind == "opcode": subs.append(toks is not None)       # the shares count every substitution; the twin runs each distinct byte-code once
                if code in seen: continue
                seen.add(code)
                secs.append((side, env, code, masks)); kinds.append(kind)
                wants.append(None if toks is None else model_rows(toks, env, masks) if toks else "empty")
    share = sum(subs) / len(subs)
    print("mutation sweep: %d distinct mutants, %d opcode substitutions of which %.1f%% decode and %.1f%% are refused" % (len(secs), len(subs), 100 * share, 100 * (1 - share)))
    assert share >= 0.25 and 1 - share >= 0.25
    assert {k for k in kinds} == {"truncate", "opcode", "operand"} and any(w is not None for w, k in zip(wants, kinds) if k == "operand")
    got = run_twin(twin_asan, tmp_path, secs)
    bad = [(i, kinds[i], secs[i][2].hex()) for i, (g, w) in enumerate(zip(got, wants)) if (g != w if w != "empty" else g is None)]
    assert not bad, (len(bad), bad[:5])
