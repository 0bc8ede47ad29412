"""CPU tests of the structured G1 arguments of the pairing tests (g1_pairing_args.py): the builders' own premises on Python integers, the
plain-C oracle against the compiled reference on exactly these inputs (replayed from tests/golden/reference_calls.bin where the reference
is absent), and the algebra the GPU and host-sim tests lean on — checked on oracle values alone, so that a later mismatch on the device is
known to be the kernel's."""
import g1_pairing_args as ga

ONE = ga.ONE


def _pairs():
    """every distinct (G1, G2) pair of the 63-lane pattern, then the placed point of each class against the placement's G2 point"""
    pairs = ga.distinct(ga.pattern())
    return pairs + [(n, "q1") for n in ga.PLACED if (n, "q1") not in pairs]


def test_builders_hold_their_premises():
    assert ga.self_check()
    lanes = ga.pattern()
    assert len(lanes) == 3 * ga.TRI and len(ga.distinct(lanes)) <= 40
    assert {a for a, _ in lanes[2 * ga.TRI:]} == set(ga.DEGENERATE) and set(ga.DEGENERATE) >= {n for c, ns in ga.CLASSES.items() for n in ns if c != "ordinary"}
    assert (ga.BIG + ga.TRI - 1) // ga.TRI == ga.QUEUE_WAVES + 1 and ga.BIG % ga.TRI == 1
    for n in ga.RAGGED:
        assert len(ga.ragged(n)) == n and ga.ragged(n)[-1][0] == "t3a"
    for name in ga.PLACED:
        pl = ga.placement(name)
        assert len(pl) == ga.TRI + 1 and pl[0] == pl[ga.TRI - 1] == pl[ga.TRI] and pl[0][0] == name
    assert all(any(n in ga.PLACED for n in names) for names in ga.CLASSES.values())
    assert ga.coverage_complete()


def test_column_patterns_walk_the_mask_word():
    """every single column at infinity, all, all but one, alternating either way, all of order 3, the cancelling pair alone and with
    live columns beside it, one off-curve element — for K = 1, 2, 3, 8, each column's entry from the four kinds"""
    for K in ga.KS:
        pats = ga.column_patterns(K)
        labels = [p[0] for p in pats]
        assert len(set(labels)) == len(labels) and all(len(cols) == K for _, cols, _ in pats)
        masks = {sum(1 << c for c in range(K) if cols[c] in ("inf", ga.OFF_CURVE)) for _, cols, _ in pats}
        full = (1 << K) - 1
        assert {1 << c for c in range(K)} <= masks and {0, full} <= masks                      # each single column, none, all
        assert {full ^ 1, full ^ (1 << (K - 1))} <= masks                                      # all but one
        assert {sum(1 << c for c in range(K) if c % 2 == b) for b in (0, 1)} <= masks          # alternating, both phases
        assert sum(1 for p in pats if "off" in p[2]) == (1 if K == 1 else 2)
        kinds = {("inf" if n == "inf" else "t3" if n.startswith("t3") else "neg" if n.startswith("-") else "ord")
                 for _, cols, _ in pats for n in cols if n != ga.OFF_CURVE}
        assert kinds == {"inf", "t3", "neg", "ord"}
        if K >= 2:
            assert sum(1 for p in pats if "gt_one_twin" in p[2]) == 2 and ga.column_g2(K, True)[0] == ga.column_g2(K, True)[1]
        assert len(set(ga.column_g2(K, False))) == K
        assert len(ga.column_bytes(K)) == 96 * K * len(pats)


def test_port_matches_reference_on_g1_pairing_arguments(oracle_port, oracle_ref):
    """Miller value and pairing of every distinct pair: the C restatement against the compiled reference"""
    pairs = _pairs()
    a, b = ga.lane_bytes(pairs)
    labels = ["%s,%s" % p for p in pairs]
    assert ga.differs(oracle_port.miller(a, b), oracle_ref.miller(a, b), 576, labels) == ""
    assert ga.differs(oracle_port.pair(a, b), oracle_ref.pair(a, b), 576, labels) == ""
    # pair_eq with the pairs against their rotation, against themselves, and with both G1 arguments at infinity
    n = len(pairs)
    a1, a2 = a + a + bytes(96) * 2, b + b + b[:384]
    c1, c2 = ga.rot(a, 96, 5) + a + bytes(96) * 2, ga.rot(b, 192, 3) + b + b[384:768]
    eq = oracle_ref.pair_eq(a1, a2, c1, c2)
    assert oracle_port.pair_eq(a1, a2, c1, c2) == eq and 0 in eq[:n] and eq[-2:] == b"\x01\x01"
    # equal sides compare equal, except where the value is the zero element: the reference multiplies by the conjugate and looks for 1
    assert [pairs[i] for i in range(n) if eq[n + i] != 1] == [("t3a", "inf2")]


def test_compressed_forms_decode_to_the_points(oracle_port):
    """the 49-byte forms the GPU test feeds: tag 2 | parity of y, x (for the smallest x also x + p) — decoded by the oracle to the same
    96 bytes, (0, 2) and (0, p - 2) among them"""
    names = list(ga.points())
    c = b"".join(ga.compress(k) for k in names)
    assert oracle_port.g1_decompress(c) == (b"".join(ga.enc(k) for k in names), b"\x01" * len(names))
    assert oracle_port.g1_compress(b"".join(ga.enc(k) for k in names)) == c
    for k in ("xmin+", "xmin-"):
        assert ga.compress(k, add_p=True) != ga.compress(k) and oracle_port.g1_decompress(ga.compress(k, add_p=True)) == (ga.enc(k), b"\x01")


def test_algebra_of_the_degenerate_arguments(oracle_port):
    """on oracle values alone: the cofactor part of G + T3 changes the Miller value and not the pairing; an order-3 point pairs to 1
    though its Miller value is not 1; P and -P cancel; the points that share y do not share a pairing; infinity gives 1 both times"""
    pairs = _pairs()
    a, b = ga.lane_bytes(pairs)
    mil = dict(zip(pairs, (oracle_port.miller(a, b)[576 * i:576 * i + 576] for i in range(len(pairs)))))
    gt = dict(zip(pairs, (oracle_port.pair(a, b)[576 * i:576 * i + 576] for i in range(len(pairs)))))
    assert oracle_port.fexp(b"".join(mil[p] for p in pairs)) == b"".join(gt[p] for p in pairs)
    for q in ("q1", "q4"):
        x, y = ga.lane_bytes([("g+t3", q), ("g", q), ("t3a", q), ("t3b", q), ("-g", q), ("b0", q), ("b1", q), ("b2", q), ("-b0", q), ("inf", q)])
        m, e = [oracle_port.miller(x, y)[576 * i:576 * i + 576] for i in range(10)], [oracle_port.pair(x, y)[576 * i:576 * i + 576] for i in range(10)]
        assert e[0] == e[1] and m[0] != m[1], q
        assert e[2] == ONE and e[3] == ONE and m[2] != ONE and m[3] != ONE and m[2] != m[3], q
        assert oracle_port.gt_op("mul", e[1], e[4]) == ONE and oracle_port.gt_op("mul", e[5], e[8]) == ONE, q
        assert e[1] != ONE and e[4] != e[1], q
        assert len({e[5], e[6], e[7]}) == 3 and len({m[5], m[6], m[7]}) == 3, q
        assert e[9] == ONE and m[9] == ONE, q
    assert gt["g+t3", "q0"] == oracle_port.pair(ga.enc("g"), ga.g2_points()["q0"]) and gt["inf", "q6"] == ONE
    assert gt["t3a", "q5"] == ONE and gt["t3b", "q7"] == ONE
    # against G2 infinity the addition lines are (0, 0, -px): px = 0 makes the line, the Miller value and the "pairing" the zero element
    assert mil["t3a", "inf2"] == bytes(576) and gt["t3a", "inf2"] == bytes(576)


def test_column_claims_hold_on_oracle_values(oracle_port):
    """what the column patterns claim — a Miller value of exactly 1, a GT value of exactly 1, the same with the cancelling pair on one
    G2 point — holds for the oracle's products; a pattern without the claim does not give 1"""
    mils = ga.Millers(oracle_port)
    for K in ga.KS:
        pats = ga.column_patterns(K)
        for twin in (False, True):
            prod = mils.product(K, twin)
            for (label, _, claims), m in zip(pats, prod):
                e = oracle_port.fexp(m)
                assert (m == ONE) == ("one" in claims), (K, twin, label)
                want_one = "gt_one" in claims or "one" in claims or (twin and "gt_one_twin" in claims)
                assert (e == ONE) == want_one, (K, twin, label)
