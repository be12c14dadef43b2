"""The rows `ipa_prepare_kernel` (mina_bridge_amd/csrc/api_ipa.hip) must leave for the combined MSM of the opening check, restated on plain Python integers from
what oracle/ already has (ipa_ref.FqSponge / shift_scalar, pasta_ref.challenge_to_field / BWParams.to_group / b_poly / endo_r).  TEST INFRASTRUCTURE ONLY.

Per proof b, with rho = rand_base^(b + pow_first), sigma = sg_rand_base^(b + pow_first), the transcript's challenges chal_j, c and U = to_group(t), the list is

    [h, sg, U, delta, L_0, R_0, .., L_{k-1}, R_{k-1}, comm_0 ..]
     h: -rho z2      sg: -rho z1 - sigma      U: -rho z1 b0 + rho c cip      delta: rho      L_j: rho c / chal_j      R_j: rho c chal_j      comm_i: rho c xi^i

An expanded slot stands as its eight (point_j, rho c xi^i * scalar_j) terms, an overridden commitment is taken from the override list, lists shorter than the
longest of the batch are padded with infinity.  Entries whose point the whole batch shares keep a ZERO scalar in the proof's list, their real scalar goes to a side
matrix, and the point stands once behind all lists (proof 0's copy of it) with the sum of the batch's scalars; `restore` gives a range of proofs theirs back.

A proof is given as a dict of integers that are NOT reduced here: k, lr (k pairs of points), delta, sg, z1, z2, evalpoints, comms, cip, polyscale, evalscale,
sponge_state (3), sponge_mode, sponge_count; a point is (x, y) or None = infinity = the encoding (0, 0).  A proof is malformed if a scalar or a sponge-state word is
not below its modulus, or a point has a coordinate not below p or is off the curve and not (0, 0); its own rows are then unspecified, everybody else's are not."""
import numpy as np

from oracle import ipa_ref as I
from oracle import pasta_ref as R

IPA_EXPAND = 8


def _pt_ok(pt, p):
    if pt is None or pt == (0, 0):
        return True
    x, y = pt
    return x < p and y < p and (y * y - x * x * x - R.CURVE_B) % p == 0


def _red(pt, p):
    if pt is None or (pt[0] % p == 0 and pt[1] % p == 0):
        return None
    return (pt[0] % p, pt[1] % p)


def ipa_rows(curve, pp, h, proofs, rand_base, sg_rand_base, pow_first=0, override_slot=None, comm_override=None, expand_slot=None, expand_point0=None,
             expand_points=None, expand_scalars=None, shared_mask=0, shared_h=0, shared_expand0=0):
    """-> dict: per, nshared, points / scalars (batch * per + nshared entries), chals [batch][k], sigma [batch], side [batch][nshared], offsets [nshared],
    malformed (any proof), malformed_each [batch]"""
    r, p = R.scalar_modulus(curve), R.base_modulus(curve)
    endo, bw = R.endo_r(curve), R.BWParams(p)
    batch, k = len(proofs), proofs[0]["k"]
    m = max(len(e["comms"]) for e in proofs)
    per = 2 * k + m + 4 + (IPA_EXPAND - 1 if expand_slot is not None else 0)
    shared_expand0 = 1 if (shared_expand0 and expand_slot is not None) else 0
    nshared = bin(shared_mask).count("1") + (1 if shared_h else 0) + shared_expand0
    assert not nshared or m <= 64
    points, scalars, chals, sigmas, side, offsets, bad_each = [], [], [], [], [], [], []
    tail_points = []
    for b, e in enumerate(proofs):
        bad = any(x >= r for x in [e["z1"], e["z2"], e["cip"], e["polyscale"], e["evalscale"]] + list(e["evalpoints"])) or any(w >= p for w in e["sponge_state"])
        sp = I.FqSponge(curve, pp, [w % p for w in e["sponge_state"]], "squeezed" if e["sponge_mode"] else "absorbed", e["sponge_count"])
        cip = e["cip"] % r
        sp.absorb_fr([I.shift_scalar(curve, cip)])
        U = bw.to_group(sp.challenge_fq())
        chal = []
        for (L, Rp) in e["lr"]:
            bad = bad or not _pt_ok(L, p) or not _pt_ok(Rp, p)
            sp.absorb_g([_red(L, p)])
            sp.absorb_g([_red(Rp, p)])
            chal.append(R.challenge_to_field(sp.challenge(), endo, r))
        bad = bad or not _pt_ok(e["delta"], p) or not _pt_ok(e["sg"], p)
        sp.absorb_g([_red(e["delta"], p)])
        c = R.challenge_to_field(sp.challenge(), endo, r)
        b0, scale = 0, 1
        for pt in e["evalpoints"]:
            b0 = (b0 + scale * R.b_poly(chal, pt % r, r)) % r
            scale = scale * e["evalscale"] % r
        rho, sigma = pow(rand_base, b + pow_first, r), pow(sg_rand_base, b + pow_first, r)
        z1, z2 = e["z1"] % r, e["z2"] % r
        rho_c = rho * c % r
        row = [(h, -rho * z2 % r, bool(shared_h)), (_red(e["sg"], p), (-rho * z1 - sigma) % r, False), (U, (-rho * z1 * b0 + rho_c * cip) % r, False),
               (_red(e["delta"], p), rho, False)]
        for (L, Rp), ch in zip(e["lr"], chal):
            row.append((_red(L, p), rho_c * R.inv(ch, r) % r, False))
            row.append((_red(Rp, p), rho_c * ch % r, False))
        xi_i = 1
        for i in range(m):
            wgt = rho_c * xi_i % r
            if i == expand_slot:
                for j in range(IPA_EXPAND):
                    pt = expand_point0 if j == 0 else expand_points[b][j - 1]
                    if j:
                        bad = bad or not _pt_ok(pt, p)
                    row.append((_red(pt, p), wgt * expand_scalars[b][j] % r, j == 0 and bool(shared_expand0)))
            else:
                pt = comm_override[b] if i == override_slot else (e["comms"][i] if i < len(e["comms"]) else None)
                bad = bad or not _pt_ok(pt, p)
                row.append((_red(pt, p), wgt, bool((shared_mask >> i) & 1)))
            xi_i = xi_i * e["polyscale"] % r
        assert len(row) == per
        mine = []
        for o, (pt, sc, shared) in enumerate(row):
            points.append(pt)
            if shared and nshared:
                scalars.append(0)
                mine.append(sc)
                if b == 0:
                    tail_points.append(pt)
                    offsets.append(o)
            else:
                scalars.append(sc)
        assert len(mine) == nshared
        side.append(mine)
        chals.append(chal)
        sigmas.append(sigma)
        bad_each.append(bool(bad))
    points += tail_points
    scalars += [sum(side[b][q] for b in range(batch)) % r for q in range(nshared)]
    return {"per": per, "nshared": nshared, "points": points, "scalars": scalars, "chals": chals, "sigma": sigmas, "side": side, "offsets": offsets,
            "malformed": any(bad_each), "malformed_each": bad_each}


def restore(rows, lo, cnt):
    """the rows after proofs [lo, lo + cnt) got their own scalars of the shared points back (the tail sums and the side matrix stay)"""
    out = dict(rows)
    sc = list(rows["scalars"])
    for b in range(lo, lo + cnt):
        for q, o in enumerate(rows["offsets"]):
            sc[b * rows["per"] + o] = rows["side"][b][q]
    out["scalars"] = sc
    return out


def prefix(rows, n, r):
    """the rows of the batch made of the first n proofs alone (rho_b and sigma_b depend on b only): their lists, and the shared tail summed over those n"""
    per, ns = rows["per"], rows["nshared"]
    out = dict(rows)
    for key in ("chals", "sigma", "side", "malformed_each"):
        out[key] = rows[key][:n]
    full = len(rows["sigma"]) * per
    out["points"] = rows["points"][: n * per] + rows["points"][full:]
    out["scalars"] = rows["scalars"][: n * per] + [sum(rows["side"][b][q] for b in range(n)) % r for q in range(ns)]
    out["malformed"] = any(out["malformed_each"])
    return out


# ---- bytes: the layouts of MinaContext.selftest_ipa_rows / pack_ipa_openings
def le32(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), np.uint8)


def pt_bytes(pt):
    """(x, y) -> 64 bytes as they are (no reduction: the malformed cases need the alias encodings); None -> zeros"""
    return np.zeros(64, np.uint8) if pt is None else np.concatenate([le32(pt[0]), le32(pt[1])])


def pts_bytes(pts):
    return np.stack([pt_bytes(q) for q in pts]) if len(pts) else np.zeros((0, 64), np.uint8)


def ints_bytes(xs):
    return np.stack([le32(x) for x in xs]) if len(xs) else np.zeros((0, 32), np.uint8)


def rows_bytes(rows):
    """the model's rows in the byte layout of MinaContext.selftest_ipa_rows"""
    batch, ns = len(rows["sigma"]), rows["nshared"]
    return {"points": pts_bytes(rows["points"]), "scalars": ints_bytes(rows["scalars"]),
            "chals": np.stack([ints_bytes(c) for c in rows["chals"]]), "sigma": ints_bytes(rows["sigma"]),
            "side": np.stack([ints_bytes(s) for s in rows["side"]]).reshape(batch, ns, 32), "offsets": np.array(rows["offsets"], np.uint32)}


def to_abi(e):
    """a proof of this module -> dict of numpy buffers for MinaContext.pack_ipa_openings"""
    return {"k": e["k"], "lr": pts_bytes([q for pair in e["lr"] for q in pair]).reshape(-1), "delta": pt_bytes(e["delta"]), "sg": pt_bytes(e["sg"]),
            "z1": le32(e["z1"]), "z2": le32(e["z2"]), "n_evalpoints": len(e["evalpoints"]),
            "evalpoints": ints_bytes(e["evalpoints"]).reshape(-1) if e["evalpoints"] else np.zeros(32, np.uint8),
            "n_comms": len(e["comms"]), "comms": pts_bytes(e["comms"]).reshape(-1) if e["comms"] else np.zeros(64, np.uint8),
            "combined_inner_product": le32(e["cip"]), "polyscale": le32(e["polyscale"]), "evalscale": le32(e["evalscale"]),
            "sponge_state": ints_bytes(e["sponge_state"]).reshape(-1), "sponge_mode": e["sponge_mode"], "sponge_count": e["sponge_count"]}


def from_minted(entry, sponge):
    """an oracle instance (ipa_ref.make_instance / ipa_helpers.mint) -> a proof of this module"""
    op = entry["opening"]
    state, mode, count = sponge.raw()
    return {"k": entry["k"], "lr": list(op["lr"]), "delta": op["delta"], "sg": op["sg"], "z1": op["z1"], "z2": op["z2"], "evalpoints": list(entry["evalpoints"]),
            "comms": list(entry["comms"]), "cip": entry["combined_inner_product"], "polyscale": entry["polyscale"], "evalscale": entry["evalscale"],
            "sponge_state": list(state), "sponge_mode": mode, "sponge_count": count}


def random_proof(rng, curve, g, k, n_comms, n_evalpoints):
    """NOT a valid opening: points g[i] of the SRS (a list of tuples), every scalar and the sponge state random and canonical; `rng` is a random.Random"""
    r, p = R.scalar_modulus(curve), R.base_modulus(curve)
    pick = lambda: g[rng.randrange(len(g))]      # noqa: E731
    return {"k": k, "lr": [(pick(), pick()) for _ in range(k)], "delta": pick(), "sg": pick(), "z1": rng.randrange(r), "z2": rng.randrange(r),
            "evalpoints": [rng.randrange(r) for _ in range(n_evalpoints)], "comms": [pick() for _ in range(n_comms)], "cip": rng.randrange(r),
            "polyscale": rng.randrange(r), "evalscale": rng.randrange(r), "sponge_state": [rng.randrange(p) for _ in range(3)],
            "sponge_mode": rng.randrange(2), "sponge_count": rng.randrange(3)}
