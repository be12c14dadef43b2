"""PolishToken programs for the interpreter tests (TEST INFRASTRUCTURE ONLY): a model of kimchi's `PolishToken::evaluate`, a restatement of the
validator's rules over the engine's byte-code, and a seeded generator of named programs.

The model is written from upstream's loop ([UPSTREAM-RECALL] `if skip_count > 0 { skip_count -= 1; continue }`, `Store => cache.push(top)`,
`Load(i) => cache[i]`, `SkipIf(f, n) => if f.is_enabled() { skip_count = n; stack.push(0) }`), as tests/test_polish_semantics.py::upstream_evaluate is,
for all 19 opcodes.  It does not use oracle/kimchi_ref.py's interpreter: tests/test_polish_programs.py compares the two, which pins the oracle as well.

Three pieces of the product must agree with it: `decode_tokens` and `polish_eval_host` (mina_bridge_amd/csrc/polish.h; tests/fuzz/polish_twin.cpp, tests/test_polish_programs.py)
and the device interpreter of `ft_eval0_dev` (kimchi_dev.cuh; tests/test_gpu_polish_programs.py)."""
import random
from collections import namedtuple

from oracle import kimchi_ref as K

P_MOD, Q_MOD = K.R.P, K.R.Q
STACK, CACHE, N_FEATURES, N_COLS, N_SLOTS = 24, 8, 21, K.N_EVAL_COLS, 19
INT32_MIN = -(1 << 31)
WRAP, STEP = "wrap", "step"
# side -> (field number of the C ABI, modulus, columns a CELL may name)
SIDES = {WRAP: (1, Q_MOD, N_COLS), STEP: (0, P_MOD, N_COLS + N_SLOTS)}

Program = namedtuple("Program", "name tokens valid")        # valid: an install must accept it


class Env:
    """what a program reads: plain integers of the field `r`.  evals[col] = (at zeta, at zeta * omega); `present`: None on the wrap side (a column is a
    column), the presence mask of the 19 optional slots on the step side, where column 43 + s names slot s and evals holds the present ones in order."""
    def __init__(self, r, log2_domain, zk_rows, zeta, alpha, beta, gamma, joint, endo, mds, evals, features=0, present=None):
        self.r, self.log2_domain, self.zk_rows, self.zeta = r, log2_domain, zk_rows, zeta
        self.alpha, self.beta, self.gamma, self.joint, self.endo, self.mds, self.evals = alpha, beta, gamma, joint, endo, mds, evals
        self.features, self.present = features, present
        self.omega = K.O_domain_generator(r, log2_domain)

    def with_masks(self, features, present=None):
        e = Env.__new__(Env); e.__dict__.update(self.__dict__); e.features = features
        if present is not None: e.present = present
        return e

    def vanishes_on_zk_rows(self):
        n, acc = 1 << self.log2_domain, 1
        for i in range(n - self.zk_rows, n):
            acc = acc * (self.zeta - pow(self.omega, i, self.r)) % self.r
        return acc

    def lagrange(self, off):
        n = 1 << self.log2_domain
        row = off if off >= 0 else n - self.zk_rows if off == INT32_MIN else n - self.zk_rows + off
        d = (self.zeta - pow(self.omega, row, self.r)) % self.r
        return (pow(self.zeta, n, self.r) - 1) * pow(d, self.r - 2, self.r) % self.r


def evaluate(tokens, env) -> int:
    """upstream's loop.  LookupError: a LOAD of a slot no executed STORE filled (upstream's index panic), a CELL of an optional slot the proof does not carry"""
    r, stack, cache, skip = env.r, [], [], 0
    for t in tokens:
        if skip:
            skip -= 1
            continue
        op = t[0]
        if op == K.T_SKIP_IF:
            if (env.features >> t[1]) & 1: skip = t[2]; stack.append(0)
        elif op == K.T_SKIP_IF_NOT:
            if not (env.features >> t[1]) & 1: skip = t[2]; stack.append(0)
        elif op == K.T_ALPHA: stack.append(env.alpha)
        elif op == K.T_BETA: stack.append(env.beta)
        elif op == K.T_GAMMA: stack.append(env.gamma)
        elif op == K.T_JOINT: stack.append(env.joint)
        elif op == K.T_ENDO: stack.append(env.endo)
        elif op == K.T_MDS: stack.append(env.mds[t[1]][t[2]])
        elif op == K.T_LITERAL: stack.append(t[1] % r)
        elif op == K.T_CELL:
            col = t[1]
            if env.present is not None and col >= N_COLS:
                slot = col - N_COLS
                if not (env.present >> slot) & 1: raise LookupError("CELL of an absent optional slot")
                col = N_COLS + bin(env.present & ((1 << slot) - 1)).count("1")
            stack.append(env.evals[col][t[2]])
        elif op == K.T_DUP: stack.append(stack[-1])
        elif op == K.T_POW: stack.append(pow(stack.pop(), t[1], r))
        elif op == K.T_ADD: b = stack.pop(); stack.append((stack.pop() + b) % r)
        elif op == K.T_MUL: b = stack.pop(); stack.append(stack.pop() * b % r)
        elif op == K.T_SUB: b = stack.pop(); stack.append((stack.pop() - b) % r)
        elif op == K.T_VANISH_ZK: stack.append(env.vanishes_on_zk_rows())
        elif op == K.T_LAGRANGE: stack.append(env.lagrange(t[1]))
        elif op == K.T_STORE: cache.append(stack[-1])
        elif op == K.T_LOAD:
            if t[1] >= len(cache): raise LookupError("LOAD of an unfilled slot")
            stack.append(cache[t[1]])
        else: raise AssertionError(op)
    assert len(stack) == 1, len(stack)
    return stack[0]


def features_used(tokens):
    return sorted({t[1] for t in tokens if t[0] in (K.T_SKIP_IF, K.T_SKIP_IF_NOT)})


# ------------------------------------------------------------------------------------------------ the validator's rules, restated over the byte-code
OPERAND_BYTES = {K.T_MDS: 2, K.T_LITERAL: 32, K.T_CELL: 2, K.T_POW: 8, K.T_LAGRANGE: 4, K.T_LOAD: 2, K.T_SKIP_IF: 3, K.T_SKIP_IF_NOT: 3}
PUSHES = (K.T_ALPHA, K.T_BETA, K.T_GAMMA, K.T_JOINT, K.T_ENDO, K.T_VANISH_ZK, K.T_MDS, K.T_LITERAL, K.T_CELL, K.T_LAGRANGE, K.T_LOAD, K.T_DUP)


def decode(code: bytes, r: int, ncols: int):
    """byte-code -> tokens in `K.T_*` tuple form, or None where an install must refuse: an unknown opcode, a cut operand, an operand out of range (feature code,
    MDS index, column, row, a literal >= r, a zero skip count), a stack that underflows or passes 24, more than 8 STOREs, a LOAD at or past the STOREs so far
    (counted as if every region ran), a region that runs past the end, straddles the end of the region around it, digs below the stack it started on or does
    not net exactly one value, and a program that does not end on one value.  The empty program is accepted."""
    toks, p, depth, stores, regions = [], 0, 0, 0, []          # regions: (index of the last token, depth on entry)
    while p < len(code):
        op = code[p]; p += 1
        if op > K.T_SKIP_IF_NOT: return None
        k = OPERAND_BYTES.get(op, 0)
        if len(code) - p < k: return None
        arg = code[p:p + k]; p += k
        if op in (K.T_SKIP_IF, K.T_SKIP_IF_NOT):
            f, n = arg[0], arg[1] | arg[2] << 8
            if f >= N_FEATURES or n == 0: return None
            tok = (op, f, n)
            regions.append((len(toks) + n, depth))
        elif op == K.T_MDS:
            if arg[0] > 2 or arg[1] > 2: return None
            tok = (op, arg[0], arg[1])
        elif op == K.T_LITERAL:
            v = int.from_bytes(arg, "little")
            if v >= r: return None
            tok = (op, v)
        elif op == K.T_CELL:
            if arg[0] >= ncols or arg[1] > 1: return None
            tok = (op, arg[0], arg[1])
        elif op == K.T_POW: tok = (op, int.from_bytes(arg, "little"))
        elif op == K.T_LAGRANGE: tok = (op, int.from_bytes(arg, "little", signed=True))
        elif op == K.T_LOAD:
            tok = (op, arg[0] | arg[1] << 8)
            if tok[1] >= stores: return None
        else: tok = (op,)
        if op in (K.T_DUP, K.T_POW, K.T_STORE) and depth < 1: return None
        if op in (K.T_ADD, K.T_MUL, K.T_SUB):
            if depth < 2: return None
            depth -= 1
        if op == K.T_STORE:
            if stores >= CACHE: return None
            stores += 1
        if op in PUSHES: depth += 1
        if depth > STACK: return None
        toks.append(tok)
        while regions and regions[-1][0] == len(toks) - 1:
            if depth != regions[-1][1] + 1: return None
            regions.pop()
        if any(depth < d for _, d in regions): return None
    if regions or (toks and depth != 1): return None
    return toks


def encode(tokens) -> bytes:
    from kimchi_helpers import encode_tokens
    return encode_tokens(tokens)


# ------------------------------------------------------------------------------------------------ generator
def region(op, f, body):
    return [(op, f, len(body))] + body


def if_feature(f, e1, e2):
    """kimchi's `if_feature(f, e1, e2)`"""
    return region(K.T_SKIP_IF_NOT, f, e1) + region(K.T_SKIP_IF, f, e2) + [(K.T_ADD,)]


def horner(terms):
    """sum_i alpha^(m - i) term_i: every term weighs differently, the stack stays one above the deepest term"""
    out = list(terms[0])
    for t in terms[1:]:
        out += [(K.T_ALPHA,), (K.T_MUL,)] + list(t) + [(K.T_ADD,)]
    return out


def _draw(rng, r, ncols, room, top_stores, all_stores, budget, nest, in_region):
    """a token sequence that nets one value on a stack with `room` free slots, drawn token by token under the validator's rules.  LOADs name slots that
    STOREs outside every region have filled (so every lane can run the program); `top_stores` / `all_stores` are one-element lists, updated"""
    out, d = [], 0
    leaves = [lambda: (K.T_ALPHA,), lambda: (K.T_BETA,), lambda: (K.T_GAMMA,), lambda: (K.T_JOINT,), lambda: (K.T_ENDO,), lambda: (K.T_VANISH_ZK,),
              lambda: (K.T_MDS, rng.randrange(3), rng.randrange(3)), lambda: (K.T_LITERAL, rng.choice([0, 1, r - 1, rng.randrange(r)])),
              lambda: (K.T_CELL, rng.randrange(ncols), rng.randrange(2)), lambda: (K.T_CELL, rng.randrange(ncols), rng.randrange(2)),
              lambda: (K.T_ALPHA,), lambda: (K.T_BETA,), lambda: (K.T_GAMMA,), lambda: (K.T_MDS, rng.randrange(3), rng.randrange(3)),
              lambda: (K.T_CELL, rng.randrange(ncols), rng.randrange(2)), lambda: (K.T_CELL, rng.randrange(ncols), rng.randrange(2)),
              lambda: (K.T_CELL, rng.randrange(ncols), rng.randrange(2)), lambda: (K.T_CELL, rng.randrange(ncols), rng.randrange(2)),
              lambda: (K.T_LAGRANGE, rng.choice([0, 1, 5, -1, -2, INT32_MIN])) if rng.random() < 0.4 else (K.T_JOINT,)]        # an inversion each: kept rare
    while True:
        left = budget - len(out)
        if d >= 1 and left <= d - 1:                       # out of budget: fold down to one value
            if d == 1: return out
            out.append((rng.choice([K.T_ADD, K.T_MUL, K.T_SUB]),)); d -= 1
            continue
        x = rng.random()
        if d >= 2 and x < 0.30: out.append((rng.choice([K.T_ADD, K.T_MUL, K.T_SUB]),)); d -= 1
        elif d >= 1 and x < 0.34: out.append((K.T_POW, rng.choice([0, 1, 2, 3, 5, 7, 7, 9, (1 << 32) + 1, rng.getrandbits(64)])))
        elif d >= 1 and x < 0.42 and all_stores[0] < CACHE:
            out.append((K.T_STORE,)); all_stores[0] += 1
            if not in_region: top_stores[0] += 1
        elif d < room and x < 0.47 and d >= 1: out.append((K.T_DUP,)); d += 1
        elif d < room and x < 0.53 and top_stores[0]: out.append((K.T_LOAD, rng.randrange(top_stores[0]))); d += 1
        elif d < room and x < 0.62 and nest < 3 and left > 8:
            body = _draw(rng, r, ncols, room - d, top_stores, all_stores, rng.randrange(1, min(left - 4, 14)), nest + 1, True)
            out += region(rng.choice([K.T_SKIP_IF, K.T_SKIP_IF_NOT]), rng.randrange(N_FEATURES), body); d += 1
        elif d < room: out.append(rng.choice(leaves)()); d += 1


def random_program(rng, r, ncols, budget, room=STACK):
    return _draw(rng, r, ncols, room, [0], [0], budget, 0, False)


def programs(side, seed, domains=None):
    """the named programs of one side, the same for the same arguments.  `domains`: the log2 sizes the `lagrange` family takes its rows n - 1 and n from
    (default: 6 on the wrap side, 10 and 16 on the step side)"""
    _, r, ncols = SIDES[side]
    rng = random.Random("%s/%d" % (side, seed))
    domains = domains or ([6] if side == WRAP else [10, 16])
    cell = lambda c, row=0: (K.T_CELL, c, row)
    lit = lambda v: (K.T_LITERAL, v)
    out = []
    add = lambda name, toks, valid=True: out.append(Program(name, list(toks), valid))

    # ---- all_ops: every opcode; all nine MDS entries; every column at both rows; the literals 0, 1, r - 1 and a random one
    rnd = rng.randrange(r)
    add("all_ops/ops", horner([[(K.T_ALPHA,)], [(K.T_BETA,)], [(K.T_GAMMA,)], [(K.T_JOINT,)], [(K.T_ENDO,)], [(K.T_VANISH_ZK,)], [(K.T_MDS, 1, 2)], [lit(0)], [lit(1)], [lit(r - 1)], [lit(rnd)],
                               [cell(K.COL_W0 + 3, 1), (K.T_DUP,), (K.T_MUL,)], [cell(9), (K.T_POW, 3)], [(K.T_BETA,), (K.T_GAMMA,), (K.T_SUB,)], [(K.T_LAGRANGE, -1)],
                               [cell(20), (K.T_STORE,)], [(K.T_LOAD, 0), cell(21, 1), (K.T_MUL,)],
                               region(K.T_SKIP_IF, 2, [cell(5), lit(77), (K.T_MUL,)]), region(K.T_SKIP_IF_NOT, 4, [cell(6, 1), lit(78), (K.T_ADD,)])]))
    add("all_ops/mds", horner([[(K.T_MDS, i, j)] for i in range(3) for j in range(3)]))
    add("all_ops/cells", horner([[cell(c, row)] for c in range(ncols) for row in (0, 1)]))

    # ---- deep: the stack reaches exactly 24 and comes back to 1; eight STOREs and a LOAD of each slot; their twins one past the bound
    def stack_to(n):
        push = [rng.choice([(K.T_ALPHA,), (K.T_BETA,), cell(rng.randrange(ncols), rng.randrange(2)), lit(rng.randrange(r)), (K.T_MDS, rng.randrange(3), rng.randrange(3))]) for _ in range(n)]
        return push + [(rng.choice([K.T_ADD, K.T_MUL, K.T_SUB]),) for _ in range(n - 1)]

    def stores(n):
        return horner([[cell(rng.randrange(ncols), rng.randrange(2)), lit(rng.randrange(r)), (K.T_MUL,), (K.T_STORE,)] for _ in range(n)] +
                      [[(K.T_LOAD, s), lit(rng.randrange(r)), (K.T_MUL,)] for s in range(min(n, CACHE))])
    add("deep/stack24", stack_to(STACK))
    add("deep/cache8", stores(CACHE))
    add("deep/both", stores(CACHE)[:-1] + stack_to(STACK - 2) + [(K.T_ADD,), (K.T_ADD,)])       # 24 deep with the cache full: the sum and the last LOAD's term below 22 more
    add("deep/stack25", stack_to(STACK + 1), False)
    add("deep/cache9", stores(CACHE + 1), False)

    # ---- pow: the exponents around the 32-bit halves, on a cell, 0 and 1
    exps = [0, 1, 2, 7, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - 1]
    add("pow/edges", horner([[base, (K.T_POW, e)] for e in exps for base in (cell(rng.randrange(ncols), rng.randrange(2)), lit(0), lit(1))]))

    # ---- lagrange: rows 0, 1, n - 1, n, and the rows counted back from the zero-knowledge rows, the sentinel among them
    offs = [0, 1] + [(1 << k) - 1 for k in domains] + [1 << k for k in domains] + [-1, -2, INT32_MIN]
    add("lagrange/rows", horner([[(K.T_LAGRANGE, o)] for o in offs]))

    # ---- regions
    body = lambda j: [cell((7 * j + 3) % ncols, j & 1), lit(rng.randrange(r)), (K.T_MUL,)]
    add("regions/if_feature_all", horner([if_feature(f, body(f), [lit(rng.randrange(r)), (K.T_BETA,), (K.T_ADD,)]) for f in range(N_FEATURES)]))
    inner3 = region(K.T_SKIP_IF_NOT, 10, body(40))
    inner2 = region(K.T_SKIP_IF, 1, [(K.T_BETA,)] + inner3 + [(K.T_ADD,)])
    add("regions/nest3", [(K.T_GAMMA,)] + region(K.T_SKIP_IF_NOT, 6, [(K.T_ALPHA,)] + inner2 + [(K.T_MUL,), lit(5), (K.T_ADD,)]) + [(K.T_MUL,)])
    add("regions/length1", [cell(11)] + region(K.T_SKIP_IF, 5, [(K.T_GAMMA,)]) + [(K.T_ADD,)] + region(K.T_SKIP_IF_NOT, 3, [(K.T_ENDO,)]) + [(K.T_MUL,)])
    add("regions/ends_on_last_token", region(K.T_SKIP_IF, 7, body(41) + [(K.T_ALPHA,), (K.T_ADD,)]))
    add("regions/nested_end_on_last_token", region(K.T_SKIP_IF_NOT, 0, [cell(12, 1)] + region(K.T_SKIP_IF_NOT, 2, [(K.T_BETA,)]) + [(K.T_MUL,)] + region(K.T_SKIP_IF, 4, [lit(9)]) + [(K.T_ADD,)]))
    add("regions/back_to_back", region(K.T_SKIP_IF, 0, body(42)) + region(K.T_SKIP_IF_NOT, 8, body(43)) + [(K.T_SUB,)] + region(K.T_SKIP_IF, 6, body(44)) + region(K.T_SKIP_IF, 6, body(45)) + [(K.T_MUL,), (K.T_ADD,)])
    # STOREs inside regions: slot 0 always; features 2 and 7 decide where the two outer STOREs behind them land, and so what LOAD 1 and LOAD 2 read
    add("regions/stores", [(K.T_ALPHA,), (K.T_STORE,)] + region(K.T_SKIP_IF_NOT, 2, body(46) + [(K.T_STORE,), (K.T_LOAD, 1), (K.T_MUL,)]) + [(K.T_ADD,)] +
        region(K.T_SKIP_IF, 7, body(47) + [(K.T_STORE,)]) + [(K.T_MUL,)] + [lit(1000), (K.T_STORE,), (K.T_ADD,), cell(13), (K.T_STORE,), (K.T_ADD,)] +
        [(K.T_LOAD, 1), (K.T_MUL,), (K.T_LOAD, 2), (K.T_SUB,), (K.T_LOAD, 0), (K.T_ADD,)])

    # ---- bad_load: slot 0 is filled only where feature 6 (LookupTables) is on
    add("bad_load/feature6", [cell(14)] + region(K.T_SKIP_IF_NOT, 6, [(K.T_ALPHA,), (K.T_STORE,)]) + [(K.T_ADD,), (K.T_LOAD, 0), (K.T_MUL,)])

    # ---- long: the size of a real linearization, shorter drawn expressions chained with ADD
    toks, top, alls = [], [0], [0]
    while len(toks) < 3000:
        e = _draw(rng, r, ncols, STACK - 1, top, alls, rng.randrange(8, 60), 0, False)
        toks += e + ([(K.T_ADD,)] if toks else [])
    add("long/chain", toks)

    # ---- random
    for i in range(12):
        add("random/%d" % i, random_program(rng, r, ncols, rng.randrange(20, 90)))
    return out


def refusals(side):
    """programs an install must refuse, beyond the `deep` twins: name -> byte-code"""
    _, r, ncols = SIDES[side]
    return {"region past the end": encode([(K.T_SKIP_IF, 3, 3), (K.T_ALPHA,), (K.T_BETA,)]),
            "feature code 21": encode([(K.T_SKIP_IF_NOT, 21, 1), (K.T_ALPHA,)]),
            "literal = modulus": encode([(K.T_LITERAL, r)]),
            "column = ncols": encode([(K.T_CELL, ncols, 0)])}


# ------------------------------------------------------------------------------------------------ mutants of a program's byte-code
def token_offsets(tokens):
    """byte offset of every token's opcode, and the length of the code"""
    offs, p = [], 0
    for t in tokens:
        offs.append(p); p += 1 + OPERAND_BYTES.get(t[0], 0)
    return offs, p


def mutants(tokens, r, ncols):
    """(kind, byte-code) of every truncation, every opcode substitution and the operand edges of a program"""
    code = encode(tokens)
    offs, n = token_offsets(tokens)
    assert n == len(code)
    for cut in range(len(code)):
        yield "truncate", code[:cut]
    for o in offs:
        for op in range(19):
            if op != code[o]:
                yield "opcode", code[:o] + bytes([op]) + code[o + 1:]
    put = lambda o, b: code[:o] + bytes(b) + code[o + len(b):]
    stores = 0
    for i, (t, o) in enumerate(zip(tokens, offs)):
        op = t[0]
        if op in (K.T_SKIP_IF, K.T_SKIP_IF_NOT):
            left = len(tokens) - 1 - i
            for cnt in (0, left, left + 1):
                yield "operand", put(o + 2, cnt.to_bytes(2, "little"))
            for f in (20, 21):
                yield "operand", put(o + 1, [f])
        elif op == K.T_CELL:
            for c in (ncols - 1, ncols):
                yield "operand", put(o + 1, [c])
            for row in (1, 2):
                yield "operand", put(o + 2, [row])
        elif op == K.T_MDS:
            for v in (2, 3):
                yield "operand", put(o + 1, [v])
                yield "operand", put(o + 2, [v])
        elif op == K.T_LOAD:
            yield "operand", put(o + 1, stores.to_bytes(2, "little"))
            if stores: yield "operand", put(o + 1, (stores - 1).to_bytes(2, "little"))
        elif op == K.T_LITERAL:
            yield "operand", put(o + 1, r.to_bytes(32, "little"))
        elif op == K.T_STORE:
            stores += 1
