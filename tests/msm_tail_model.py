"""Integer restatement of the fused MSM tail (mina_bridge_amd/csrc/msm.cuh msm_tail_kernel).  The group is modelled as the integers modulo the curve's order, so
a bucket is a number and a point addition is an addition: what is left is the ORDER of the kernel's sums, step by step.

    row r of a set (one workgroup):   S_r = sum_c B[r][c],   T_r = sum_c (c + 1) B[r][c]                                  (C = 128 columns)
    set total (the last arriver):     sum_b (b + 1) B_b = sum_r T_r + C * sum_r r * S_r              with b = r C + c
    problem (the last set's arriver): Horner over the set totals, c doublings between two sets

Both weighted sums are formed as the kernel forms them (tail_weighted_block_sum): 1, 2 or 4 consecutive values per quad, the plain and weighted sum of a wave's
16 quads by a suffix scan (quadwave_weighted_sum), the four waves' results combined at the end."""

ORDER = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001      # the order of Pallas (a prime): the model's group
C = 128


def quadwave_weighted_sum(v):
    """2^k values -> (sum_q v_q, sum_q q v_q) by the suffix scan of the wave collective: v'_q = sum_{j >= q} v_j, then the sum of v'_1 .. v'_(2^k - 1)"""
    width = len(v)
    assert width in (4, 16)
    v = list(v)
    d = 1
    while d < width:
        v = [(v[q] + v[q + d]) % ORDER if q + d < width else v[q] for q in range(width)]
        d *= 2
    return v[0], sum(v[1:]) % ORDER


def weighted_block_sum(vals):
    """(sum_i v_i, sum_i i v_i) over up to 256 values, as tail_weighted_block_sum does: quad Q of 64 takes the P = 1, 2 or 4 consecutive values P Q + t and forms
    s_Q = sum_t v_t and l_Q = sum_t t v_t from suffix sums; each wave's 16 quads give (S_w, X_w) and L_w; the four waves' results are combined:
    sum_i i v_i = P (16 sum_w w S_w + sum_w X_w) + sum_w L_w"""
    n = len(vals)
    assert 1 <= n <= 256
    log2p = 0 if n <= 64 else (1 if n <= 128 else 2)
    p = 1 << log2p
    at = lambda i: vals[i] if i < n else 0
    s, l = [0] * 64, [0] * 64
    for q in range(64):
        suf = 0
        for t in range(p - 1, 0, -1):
            suf = (suf + at(p * q + t)) % ORDER
            l[q] = (l[q] + suf) % ORDER
        s[q] = (suf + at(p * q)) % ORDER
    waves = [quadwave_weighted_sum(s[16 * w:16 * w + 16]) for w in range(4)]      # (S_w, X_w)
    big_l = [sum(l[16 * w:16 * w + 16]) % ORDER for w in range(4)]
    tot, y = quadwave_weighted_sum([sw for sw, _ in waves])                        # wave 0: sum_w S_w and sum_w w S_w
    for _ in range(4):
        y = 2 * y % ORDER
    y = (y + sum(xw for _, xw in waves)) % ORDER                                   # + wave 1's sum_w X_w
    for _ in range(log2p):
        y = 2 * y % ORDER
    return tot, (y + sum(big_l)) % ORDER                                           # + wave 2's sum_w L_w


def row_pair(row):
    """one workgroup: the row's 128 buckets -> (S_r, T_r)"""
    assert len(row) == C
    s, w = weighted_block_sum(row)
    return s, (w + s) % ORDER


def set_total(buckets):
    """the R = NB / 128 workgroups of a set, then its last arriver: sum_r T_r + C * sum_r r S_r"""
    assert len(buckets) % C == 0
    pairs = [row_pair(buckets[r * C:(r + 1) * C]) for r in range(len(buckets) // C)]
    _, w = weighted_block_sum([p[0] for p in pairs])
    tt = sum(p[1] for p in pairs) % ORDER
    for _ in range(7):                            # * C
        w = 2 * w % ORDER
    return (w + tt) % ORDER


def problem_total(sets, c):
    """the workgroup that completes a problem's last set: Horner over its set totals, c doublings per step (a fixed-base problem has one set)"""
    totals = [set_total(b) for b in sets]
    t = totals[-1]
    for tot in reversed(totals[:-1]):
        for _ in range(c):
            t = 2 * t % ORDER
        t = (t + tot) % ORDER
    return t
