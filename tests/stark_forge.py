"""Forger of improvement-proof (STARK) envelopes that isolate each check of the verifier, and grammar-aware mutations of valid ones, built on
the Python oracle (oracle/py/stark.py).  Test infrastructure only.

`forge(old, new, **deviation)` restates the oracle's prover with hooks.  One deviation is applied and everything after it -- every later
challenge, opening and byte -- is computed honestly from what was actually committed, so the Fiat-Shamir chain of a forgery is intact and
exactly ONE check of the verifier can refuse it.  `forgeries(old, new)` names that check for every forgery: the envelope is rejected, it is
accepted by `stark.verify(..., skip={check})`, and it is rejected under every other single skip (tests/test_stark_forge.py).  A forgery is
therefore a statement about the verifier: one that lacks the named check accepts a false proof.

  h_shift                       the composition polynomial's constant coefficient + 1, all else consistent with it      -> "ood"
  bent_trace, wrong_first_row,  false statements proved as honestly as possible (one row moved by 1; a linear trace from old + 1, or to
  wrong_last_row                new - 1; the composition cut to its low 8 coefficients)                                  -> "ood"
  fake_rem_commit               the third commitment is the hash of other elements, the remainder sent is the true one  -> "rem_commit"
  padded_queries                one more value in both query blocks and the query count + 1; the openings are the true ones, which do not
                                look at the surplus value                                                               -> "query_count"
  fake_t_root, fake_h_root      the root sent is another digest; values and paths come from the true tree               -> "t_root" / "h_root"
  t_leaf_*, h_leaf_*            one LDE value changed before the tree is built, at the first / a middle / the last opened position k
                                                                                                                        -> ("deep", k)

`mutations(env, old)` yields envelopes that are compared with the oracle's verdict, whatever it is: every length prefix re-encoded in every
width of winter-utils' variable-length integer that holds it (all valid), the nine-byte form with a wrong value, every field element made
non-canonical, the opening's structure and the envelope's framing bent one way at a time.  `layout(env)` gives the offset and length of
every field they touch.

`PYTHONPATH=. python tests/stark_forge.py` (from the repository root) repeats the seeded searches behind the constants PAIRS and LEAF below and prints them.
"""
import collections
import contextlib
import functools
import random

from oracle.py import stark as s
from oracle.py.blake3 import blake3

P = s.P
Forgery = collections.namedtuple("Forgery", "name env old check")      # check: the one name of stark.SKIPPABLE (or ("deep", k)) that refuses it
Mutation = collections.namedtuple("Mutation", "name env old kind")      # kind: "vint_form" (valid to the oracle) or the family's name

# (old, new) -> distinct query positions of the honest proof.  (0, 1) and the top of the range, then pairs from search_pairs(): the first pair
# of its stream for each of five more counts, so that the openings' shapes (lists per level, nodes per list) differ as far as 32 draws from
# 64 rows commonly do (mean 25.4, standard deviation 2).
PAIRS = {
    (0, 1): 27,
    (2**64 - 2, 2**64 - 1): 25,
    (7802423518971212709, 7802423522867806515): 20,
    (9211604062182188228, 9211604064352365706): 22,
    (3872982626502034966, 3872982626905158819): 24,
    (8711387064946514083, 8711387067745084607): 26,
    (4157416832381507048, 4157416832458234590): 29,
}
# (old, new) -> {family: (position, delta)}: the changed LDE row of the leaf families, from search_leaf()
LEAF = {
    (0, 1): {"t_leaf_first": (0, 1), "t_leaf_middle": (31, 1), "t_leaf_last": (63, 4), "h_leaf_first": (0, 3), "h_leaf_middle": (32, 3), "h_leaf_last": (63, 1)},
    (2**64 - 2, 2**64 - 1): {"t_leaf_first": (0, 3), "t_leaf_middle": (31, 1), "t_leaf_last": (63, 1), "h_leaf_first": (0, 1), "h_leaf_middle": (31, 4), "h_leaf_last": (63, 1)},
    (7802423518971212709, 7802423522867806515): {"t_leaf_first": (0, 3), "t_leaf_middle": (31, 2), "t_leaf_last": (63, 1), "h_leaf_first": (0, 1), "h_leaf_middle": (32, 1), "h_leaf_last": (63, 1)},
    (9211604062182188228, 9211604064352365706): {"t_leaf_first": (0, 2), "t_leaf_middle": (31, 1), "t_leaf_last": (63, 1), "h_leaf_first": (0, 1), "h_leaf_middle": (32, 2), "h_leaf_last": (63, 2)},
    (3872982626502034966, 3872982626905158819): {"t_leaf_first": (1, 4), "t_leaf_middle": (31, 1), "t_leaf_last": (63, 1), "h_leaf_first": (0, 1), "h_leaf_middle": (32, 2), "h_leaf_last": (63, 2)},
    (8711387064946514083, 8711387067745084607): {"t_leaf_first": (0, 1), "t_leaf_middle": (31, 1), "t_leaf_last": (63, 1), "h_leaf_first": (0, 3), "h_leaf_middle": (31, 1), "h_leaf_last": (63, 1)},
    (4157416832381507048, 4157416832458234590): {"t_leaf_first": (0, 2), "t_leaf_middle": (31, 2), "t_leaf_last": (63, 4), "h_leaf_first": (0, 1), "h_leaf_middle": (31, 2), "h_leaf_last": (63, 2)},
}


# ---------------------------------------------------------------------------------------------- the prover, with hooks
def _digest_of(tag):
    return blake3(b"stark_forge:" + tag)


@functools.lru_cache(maxsize=None)
def _forge(old, new, h_shift, trace, fake_rem_commit, fake_t_root, fake_h_root, t_leaf, h_leaf, pad_queries):
    col, step = s.trace_column(old, new)                      # `step` is what the verifier derives from the public (old, new)
    false_statement = trace is not None
    if trace == "bent":
        col[3] = (col[3] + 1) % P
    elif trace == "first":                                    # linear from old + 1 to new
        col = [(old + 1 + i * ((new - old - 1) * s.inv(7) % P)) % P for i in range(8)]
    elif trace == "last":                                     # linear from old to new - 1
        col = [(old + i * ((new - 1 - old) * s.inv(7) % P)) % P for i in range(8)]
    else:
        assert trace is None
    coin = s.Coin(s.context_elements() + [old, new])
    g = s.root_of_unity(s.TRACE_LEN)
    # 1. trace commitment
    t_poly = s.interpolate(col)
    t_true = s.evaluate_on_coset(t_poly, s.LDE_SIZE, s.GENERATOR)
    t_lde = list(t_true)
    if t_leaf is not None:
        t_lde[t_leaf[0]] = (t_lde[t_leaf[0]] + t_leaf[1]) % P
    t_tree = s.MerkleTree([s.hash_elements([v]) for v in t_lde])
    t_root = _digest_of(b"t_root") if fake_t_root else t_tree.root
    coin.reseed(t_root)
    # 2. constraint evaluations (of the trace polynomial: a changed leaf is a lie about one row, not another polynomial)
    coef = [coin.draw() for _ in range(3)]
    w_ce = s.root_of_unity(s.CE_SIZE)
    stride = s.LDE_SIZE // s.CE_SIZE
    ce = []
    for i in range(s.CE_SIZE):
        x = s.GENERATOR * pow(w_ce, i, P) % P
        ce.append(s.constraint_evaluation(x, t_true[i * stride], t_true[(i * stride + s.BLOWUP) % s.LDE_SIZE], old, new, step, coef))
    h_full = s.interpolate(ce, s.GENERATOR)
    assert false_statement or all(c == 0 for c in h_full[s.TRACE_LEN:])
    assert not false_statement or any(h_full[s.TRACE_LEN:]), "the false statement's quotient is a polynomial"
    h_poly = h_full[:s.TRACE_LEN]
    h_poly[0] = (h_poly[0] + h_shift) % P
    h_lde = s.evaluate_on_coset(h_poly, s.LDE_SIZE, s.GENERATOR)
    if h_leaf is not None:
        h_lde[h_leaf[0]] = (h_lde[h_leaf[0]] + h_leaf[1]) % P
    h_tree = s.MerkleTree([s.hash_elements([v]) for v in h_lde])
    h_root = _digest_of(b"h_root") if fake_h_root else h_tree.root
    coin.reseed(h_root)
    # 3. out-of-domain frame
    z = coin.draw()
    tz, tzg = s.horner(t_poly, z), s.horner(t_poly, z * g % P)
    coin.reseed(s.hash_elements([tz, tzg]))
    hz = s.horner(h_poly, z)
    coin.reseed(s.hash_elements([hz]))
    # 4. DEEP composition polynomial
    deep = [coin.draw() for _ in range(2)]
    t1 = s.syn_div([(t_poly[0] - tz) % P] + t_poly[1:], z)
    t2 = s.syn_div([(t_poly[0] - tzg) % P] + t_poly[1:], z * g % P)
    c1 = s.syn_div([(h_poly[0] - hz) % P] + h_poly[1:], z)
    d_poly = [(deep[0] * (a + b) + deep[1] * c) % P for a, b, c in zip(t1, t2, c1)] + [0]
    # 5. FRI remainder
    remainder = d_poly[:s.LDE_SIZE // s.BLOWUP]
    rem_commit = s.hash_elements([(remainder[0] + 1) % P] + remainder[1:]) if fake_rem_commit else s.hash_elements(remainder)
    coin.reseed(rem_commit)
    # 6. queries
    positions = sorted(set(coin.draw_integers(s.NUM_QUERIES, s.LDE_SIZE, 0)))
    depth = s.LDE_SIZE.bit_length() - 1
    surplus = [s.el_bytes(1)] * pad_queries
    tq = s._queries_bytes([s.el_bytes(t_lde[p]) for p in positions] + surplus, t_tree.prove_batch(positions), depth)
    cq = s._queries_bytes([s.el_bytes(h_lde[p]) for p in positions] + surplus, h_tree.prove_batch(positions), depth)
    # 7. serialisation
    commitments = t_root + h_root + rem_commit
    ood_trace = bytes([2]) + s.el_bytes(tz) + s.el_bytes(tzg)
    ood_eval = s.el_bytes(hz)
    rem_bytes = b"".join(s.el_bytes(c) for c in remainder)
    out = (s.context_bytes() + bytes([len(positions) + pad_queries]) + len(commitments).to_bytes(2, "little") + commitments + tq + cq +
           len(ood_trace).to_bytes(2, "little") + ood_trace + len(ood_eval).to_bytes(2, "little") + ood_eval +
           bytes([0]) + len(rem_bytes).to_bytes(2, "little") + rem_bytes + bytes([1]) + (0).to_bytes(8, "little") + bytes([0]))
    return out, tuple(positions)


def forge(old, new, *, h_shift=0, trace=None, fake_rem_commit=False, fake_t_root=False, fake_h_root=False, t_leaf=None, h_leaf=None,
          pad_queries=0, detail=None):
    """The bare proof bytes of oracle.prove(old, new) under one deviation (none: the honest proof, byte for byte).
    trace: "bent" | "first" | "last"; t_leaf / h_leaf: (position, delta) added to one LDE row before its tree is built."""
    out, positions = _forge(old, new, h_shift, trace, fake_rem_commit, fake_t_root, fake_h_root, t_leaf, h_leaf, pad_queries)
    if detail is not None:
        detail["positions"] = list(positions)
    return out


def envelope(old, new, proof, commitment=None):
    payload = old.to_bytes(8, "little") + new.to_bytes(8, "little") + proof
    commitment = s.commit_improvement(old, new) if commitment is None else commitment
    return bytes([2, 5]) + len(payload).to_bytes(4, "little") + len(commitment).to_bytes(4, "little") + payload + commitment


# ---------------------------------------------------------------------------------------------- the forgeries
LEAF_FAMILIES = tuple("%s_leaf_%s" % (t, w) for t in "th" for w in ("first", "middle", "last"))


def _leaf_index(old, new, family, pos, delta):
    """k such that `pos` is the k-th opened position of the forgery, if it is where the family wants it; else None"""
    d = {}
    forge(old, new, **{family[:6]: (pos, delta)}, detail=d)
    q = d["positions"]
    if pos not in q:
        return None
    k, where = q.index(pos), family[7:]
    ok = k == 0 if where == "first" else k == len(q) - 1 if where == "last" else 0 < k < len(q) - 1
    return k if ok else None


def search_leaf(old, new, family):
    """(position, delta) from the wanted end of the domain: the change moves the root, the root moves the positions, so whether the changed
    row is opened (and where) is only known after the fact.  A row is opened with probability 0.4: a handful of forge calls."""
    order = {"first": range(64), "last": range(63, -1, -1), "middle": sorted(range(64), key=lambda p: abs(2 * p - 63))}[family[7:]]
    for pos in order:
        for delta in range(1, 5):
            if _leaf_index(old, new, family, pos, delta) is not None:
                return pos, delta
    raise AssertionError("no opened position found")


def search_pairs(seed=1, want=(20, 22, 24, 26, 29)):
    """the first (old, new) of a seeded stream for every count of distinct positions in `want`"""
    rnd, found = random.Random(seed), {}
    while len(found) < len(want):
        old = rnd.randrange(2**63)
        new = old + 1 + rnd.randrange(2**32)
        d = {}
        forge(old, new, detail=d)
        if len(d["positions"]) in want:
            found.setdefault(len(d["positions"]), (old, new))
    return [found[c] for c in want]


def forgeries(old, new):
    """Every forgery for one (old, new) of PAIRS: [Forgery].  Asserts that the honest restatement is the oracle's prover byte for byte and
    that each recorded leaf still lands where its family says."""
    assert forge(old, new) == s.prove(old, new)
    mk = lambda name, check, **dev: Forgery(name, envelope(old, new, forge(old, new, **dev)), old, check)  # noqa: E731
    out = [mk("h_shift", "ood", h_shift=1), mk("bent_trace", "ood", trace="bent"), mk("wrong_first_row", "ood", trace="first"),
           mk("wrong_last_row", "ood", trace="last"), mk("fake_rem_commit", "rem_commit", fake_rem_commit=True),
           mk("fake_t_root", "t_root", fake_t_root=True), mk("fake_h_root", "h_root", fake_h_root=True)]
    if PAIRS[(old, new)] < s.NUM_QUERIES:
        out.append(mk("padded_queries", "query_count", pad_queries=1))
    for family in LEAF_FAMILIES:
        pos, delta = LEAF[(old, new)][family]
        k = _leaf_index(old, new, family, pos, delta)
        assert k is not None, (old, new, family)
        out.append(mk(family, ("deep", k), **{family[:6]: (pos, delta)}))
    return out


# ---------------------------------------------------------------------------------------------- the grammar
def vint_width(buf, pos):
    first = buf[pos]
    return 9 if first == 0 else (first & -first).bit_length()


def vint_w(v, w):
    """v in the w-byte form of winter-utils' variable-length usize (w = 9: a zero byte, then the value's 8 bytes)"""
    if w == 9:
        return b"\0" + v.to_bytes(8, "little")
    assert 1 <= w <= 8 and v < 1 << (7 * w)
    return (((v << 1) | 1) << (w - 1)).to_bytes(w, "little")


def layout(env):
    """{field name: (offset, length)} of a well-formed improvement envelope, in envelope order, read from its own length fields.
    Query blocks are "t" (trace) and "h" (composition): <b>.block, <b>.values_len (a vint), <b>.value<i>, <b>.open_len (vint), <b>.opening,
    <b>.depth, <b>.nlists (vint), <b>.list<k> (count byte and nodes), <b>.list<k>.count, <b>.list<k>.node<j>."""
    L, pos = collections.OrderedDict(), 0

    def put(name, n):
        nonlocal pos
        L[name] = (pos, n)
        pos += n

    for name, n in (("version", 1), ("scheme", 1), ("plen", 4), ("clen", 4), ("old", 8), ("new", 8), ("context", 28), ("nq", 1),
                    ("commitments_len", 2), ("t_root", 32), ("h_root", 32), ("rem_commit", 32)):
        put(name, n)
    nq = env[L["nq"][0]]
    for b in "th":
        start = pos
        put(b + ".values_len", vint_width(env, pos))
        nbytes, _ = s.read_vint(env, L[b + ".values_len"][0])
        assert nbytes == 16 * nq
        for i in range(nq):
            put("%s.value%d" % (b, i), 16)
        put(b + ".open_len", vint_width(env, pos))
        olen, _ = s.read_vint(env, L[b + ".open_len"][0])
        L[b + ".opening"] = (pos, olen)
        put(b + ".depth", 1)
        put(b + ".nlists", vint_width(env, pos))
        nlists, _ = s.read_vint(env, L[b + ".nlists"][0])
        for k in range(nlists):
            cnt = env[pos]
            L["%s.list%d" % (b, k)] = (pos, 1 + 32 * cnt)
            put("%s.list%d.count" % (b, k), 1)
            for j in range(cnt):
                put("%s.list%d.node%d" % (b, k, j), 32)
        assert pos == sum(L[b + ".opening"])
        L[b + ".block"] = (start, pos - start)
    for name, n in (("ood_trace_len", 2), ("ood_frame", 1), ("tz", 16), ("tzg", 16), ("ood_eval_len", 2), ("hz", 16), ("fri_layers", 1),
                    ("rem_len", 2)):
        put(name, n)
    for i in range(8):
        put("rem%d" % i, 16)
    for name, n in (("fri_partitions", 1), ("nonce", 8), ("gkr", 1), ("commitment", 32)):
        put(name, n)
    assert pos == len(env) and int.from_bytes(env[2:6], "little") == pos - 42
    return L


def splice(env, edits, plen=True):
    """env with [(offset, length, replacement)] applied (the edits do not overlap); plen: the payload length is set to what the result holds"""
    out = bytearray(env)
    for off, ln, new in sorted(edits, reverse=True):
        out[off:off + ln] = new
    if plen:
        out[2:6] = (len(out) - 42).to_bytes(4, "little")
    return bytes(out)


def _grow_opening(L, b, by):
    """the edit that adjusts block b's opening byte count (kept in its width where it fits)"""
    off, w = L[b + ".open_len"]
    v = L[b + ".opening"][1] + by
    return (off, w, vint_w(v, w) if w == 9 or v < 1 << (7 * w) else s.vint(v))


PREFIXES = tuple(b + p for b in "th" for p in (".values_len", ".open_len", ".nlists"))


def _reencode(env, L, name, v, w):
    off, cur = L[name]
    edits = [(off, cur, vint_w(v, w))]
    if name.endswith(".nlists"):
        edits.append(_grow_opening(L, name[0], w - cur))
    return splice(env, edits)


def vint_forms(env, old):
    """every length prefix in every other width that holds its value, the enclosing lengths adjusted: all valid to the oracle"""
    L, out = layout(env), []
    for name in PREFIXES:
        v, _ = s.read_vint(env, L[name][0])
        for w in range(1, 10):
            if w != L[name][1] and (w == 9 or v < 1 << (7 * w)):
                out.append(Mutation("%s:%d_bytes" % (name, w), _reencode(env, L, name, v, w), old, "vint_form"))
    return out


def vint_values(env, old):
    """the nine-byte form with a value that is wrong above bit 31, above bit 62, and everywhere: a reader that keeps fewer than 64 bits of the
    value takes the first for the right one"""
    L, out = layout(env), []
    for name in PREFIXES:
        v, _ = s.read_vint(env, L[name][0])
        for tag, bad in (("plus_2^32", v + 2**32), ("plus_2^63", v + 2**63), ("2^64-1", 2**64 - 1)):
            out.append(Mutation("%s:%s" % (name, tag), _reencode(env, L, name, bad, 9), old, "vint_value"))
    return out


def element_fields(L):
    return [n for n in L if ".value" in n and not n.endswith("_len")] + ["tz", "tzg", "hz"] + ["rem%d" % i for i in range(8)]


def noncanonical_elements(env, old):
    L, out = layout(env), []
    names = element_fields(L)
    assert len(names) == 2 * env[L["nq"][0]] + 11
    for name in names:
        for tag, v in (("p", P), ("p+1", P + 1), ("2^128-1", 2**128 - 1)):
            out.append(Mutation("%s:%s" % (name, tag), splice(env, [(L[name][0], 16, v.to_bytes(16, "little"))]), old, "element"))
    return out


def structure_mutations(env, old):
    L, out = layout(env), []
    cut = lambda name: env[L[name][0]:sum(L[name])]  # noqa: E731
    add = lambda name, e: out.append(Mutation(name, e, old, "structure"))  # noqa: E731
    for b in "th":
        nlists, _ = s.read_vint(env, L[b + ".nlists"][0])
        nl_off, nl_w = L[b + ".nlists"]
        # a node moved from one list to its neighbour (the first list that has one, to the list after it or before it)
        k = next(k for k in range(nlists) if env[L["%s.list%d.count" % (b, k)][0]] > 0)
        to = k + 1 if k + 1 < nlists else k - 1
        src, dst = "%s.list%d" % (b, k), "%s.list%d" % (b, to)
        node = cut(src)[-32:]
        add(b + ":node_moved_to_neighbour", splice(env, [(L[src][0], L[src][1], bytes([env[L[src][0]] - 1]) + cut(src)[1:-32]),
                                                       (L[dst][0], L[dst][1], bytes([env[L[dst][0]] + 1]) + cut(dst)[1:] + node)]))
        last = "%s.list%d" % (b, nlists - 1)
        add(b + ":node_appended_to_last_list", splice(env, [(L[last][0], L[last][1], bytes([env[L[last][0]] + 1]) + cut(last)[1:] + node),
                                                          _grow_opening(L, b, 32)]))
        add(b + ":last_list_dropped", splice(env, [(L[last][0], L[last][1], b""), (nl_off, nl_w, vint_w(nlists - 1, nl_w)),
                                                 _grow_opening(L, b, -L[last][1])]))
        add(b + ":last_list_dropped_count_kept", splice(env, [(L[last][0], L[last][1], b""), _grow_opening(L, b, -L[last][1])]))
        for d in (-1, 1):
            add("%s:nlists%+d" % (b, d), splice(env, [(nl_off, nl_w, vint_w(nlists + d, nl_w))]))
        for depth in (5, 7):
            add("%s:depth_%d" % (b, depth), splice(env, [(L[b + ".depth"][0], 1, bytes([depth]))]))
    nq = env[L["nq"][0]]
    for d in (-1, 1):
        add("nq%+d" % d, splice(env, [(L["nq"][0], 1, bytes([nq + d]))]))
    add("query_blocks_swapped", splice(env, [(L["t.block"][0], L["t.block"][1], cut("h.block")), (L["h.block"][0], L["h.block"][1], cut("t.block"))]))
    add("tz_tzg_swapped", splice(env, [(L["tz"][0], 16, cut("tzg")), (L["tzg"][0], 16, cut("tz"))]))
    for i in (0, 7):
        add("nonce_byte%d" % i, splice(env, [(L["nonce"][0] + i, 1, b"\1")]))
    add("gkr_byte", splice(env, [(L["gkr"][0], 1, b"\1")]))
    end = L["commitment"][0]
    add("extra_byte_plen_adjusted", splice(env, [(end, 0, b"\0")]))
    add("extra_byte", splice(env, [(end, 0, b"\0")], plen=False))
    add("extra_byte_after_commitment", env + b"\0")
    return out


def framing_mutations(env, old):
    L, out = layout(env), []
    new = int.from_bytes(env[L["new"][0]:sum(L["new"])], "little")
    plen = len(env) - 42
    add = lambda name, e, o=old: out.append(Mutation(name, e, o, "framing"))  # noqa: E731
    hdr = lambda p, c: env[:2] + p.to_bytes(4, "little") + c.to_bytes(4, "little")  # noqa: E731
    for c in (31, 33):
        add("clen_%d_header_only" % c, hdr(plen, c) + env[10:])
    add("clen_31", hdr(plen, 31) + env[10:-1])
    add("clen_33", hdr(plen, 33) + env[10:] + b"\0")
    for d in (-1, 1):
        add("plen%+d" % d, hdr(plen + d, 32) + env[10:])
    add("plen+1_clen_31", hdr(plen + 1, 31) + env[10:])                      # the same bytes, the boundary moved into the commitment
    add("plen-1_clen_33", hdr(plen - 1, 33) + env[10:])
    proof = env[26:L["commitment"][0]]
    add("new_equals_old", envelope(old, old, proof))
    add("new_below_old", envelope(new, old, proof), new)
    add("commitment_of_another_pair", envelope(old, new, proof, s.commit_improvement(old, new + 1)))
    o2, n2 = (old + 1, new) if old + 1 < new else (old, new + 1)          # the proof under another pair's own, consistent framing
    add("another_pair_with_its_commitment", envelope(o2, n2, proof), o2)
    add("version_1", b"\1" + env[1:])
    add("scheme_3", env[:1] + b"\3" + env[2:])
    return out


def mutations(env, old):
    return vint_forms(env, old) + vint_values(env, old) + noncanonical_elements(env, old) + structure_mutations(env, old) + framing_mutations(env, old)


# ---------------------------------------------------------------------------------------------- the list both test tiers run
Case = collections.namedtuple("Case", "name env old kind want")         # kind: "honest" | "forgery" | a Mutation's kind; want: the oracle's verdict
MUTATED_IN_FULL, MUTATED_WITHOUT_ELEMENTS = (0, 1), (7802423518971212709, 7802423522867806515)     # 27 and 20 opened positions


@contextlib.contextmanager
def memoised_hash():
    """The oracle's BLAKE3 (pure Python, most of a verification's time) behind a cache: the envelopes here share nearly all their hashes."""
    plain = s.blake3
    s.blake3 = functools.lru_cache(maxsize=None)(plain)
    try:
        yield
    finally:
        s.blake3 = plain


@functools.lru_cache(maxsize=None)
def corpus():
    """Every forgery of every pair and the mutations of two honest envelopes, an honest envelope after every third of them, each with the
    oracle's verdict: [Case].  Built once per process."""
    with memoised_hash():
        honest = [(s.prove_improvement(o, n), o) for o, n in PAIRS]
        bad = [Case("%s(%d,%d)" % (f.name, o, n), f.env, f.old, "forgery", None) for o, n in PAIRS for f in forgeries(o, n)]
        for (o, n), drop in ((MUTATED_IN_FULL, ()), (MUTATED_WITHOUT_ELEMENTS, ("element",))):
            bad += [Case("%s(%d,%d)" % (m.name, o, n), m.env, m.old, m.kind, None) for m in mutations(s.prove_improvement(o, n), o) if m.kind not in drop]
        out = []
        for i, c in enumerate(bad):
            out.append(c._replace(want=s.verify_improvement(c.env, c.old)))
            if i % 3 == 2:
                env, o = honest[(i // 3) % len(honest)]
                out.append(Case("honest(%d)" % o, env, o, "honest", s.verify_improvement(env, o)))
    return out


if __name__ == "__main__":
    pairs = [(0, 1), (2**64 - 2, 2**64 - 1)] + search_pairs()
    counts = {}
    for o, n in pairs:
        d = {}
        forge(o, n, detail=d)
        counts[(o, n)] = len(d["positions"])
    print("PAIRS = {\n%s}" % "".join("    (%d, %d): %d,\n" % (o, n, c) for (o, n), c in counts.items()))
    print("LEAF = {\n%s}" % "".join("    (%d, %d): {%s},\n" % (o, n, ", ".join('"%s": (%d, %d)' % ((f,) + search_leaf(o, n, f)) for f in LEAF_FAMILIES))
                                   for o, n in pairs))
