"""CPU tests of the crafted case list of tests/paillier_dec_branch_cases.py: the word model's per-site records (tools/paillier_dec_model.py)
show every (site, branch) the list claims — which keeps tests/test_gpu_paillier_dec_branches.py from passing vacuously —, the word model
agrees with the definitions on every item, every claimed item would expose the defect that belongs to its branch (the word model with that
one line of pd_mod removed computes other outputs), and random operands do not reach the add-back: why the list is needed."""
import functools
import random

import pytest

import helpers as H
import paillier_dec_branch_cases as BC
import paillier_dec_model as M

W = BC.W
FAULT_OF = {"addback": "no_addback", "overflow": "no_overflow_clause", "break": "no_rh_break"}
_is_prime = functools.lru_cache(maxsize=None)(H.is_probable_prime)


def batches():
    return dict(BC.list_1024() + [("wide 2048", BC.wide(2048)), ("wide 4096", BC.wide(4096))])


NAMES = ["split 0", "split 1", "finish 0", "crt 0", "crt 1", "keys 0", "wide 2048", "wide 4096"]


def _key(b, i):
    return b["keys"][i if len(b["keys"]) > 1 else 0]


@functools.lru_cache(maxsize=None)
def records(name, i):
    """(outputs, per-site records) of item i by the word model"""
    b = batches()[name]
    sites = {}
    return W.open_words(*_key(b, i), b["c"][i], b["n_bits"] // 64, sites), sites


def holds(st, branch):
    if branch.startswith("addback@"):
        return int(branch[8:]) in st["addback_at"]
    return {"overflow": st["overflows"] > 0, "break": st["breaks"] > 0, "two_turns": st["max_loops"] >= 2}[branch]


def test_the_names_are_the_list_s():
    assert list(batches()) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_site_records_show_every_claimed_branch(name):
    b = batches()[name]
    assert b["crafted"] and len(b["c"]) <= 50
    for i in b["crafted"]:
        got, sites = records(name, i)
        for site, branch in b["claims"][i]:
            assert site in sites and holds(sites[site], branch), (b["tag"][i], site, branch, sites.get(site))
        # every crafted item between ordinary encrypted neighbours
        assert b["tag"][i - 1] == "ordinary" and b["tag"][i + 1] == "ordinary" and b["truth"][i - 1] and b["truth"][i + 1]
        # at the split the two lanes of an item do not both take the add-back
        assert not (sites.get("split_sq_p", {}).get("addbacks") and sites.get("split_sq_q", {}).get("addbacks")), b["tag"][i]
    for i in range(len(b["c"])):
        if b["tag"][i] == "ordinary":                           # the neighbours take no add-back anywhere
            assert not any(st.get("addbacks") for st in records(name, i)[1].values())


def _claimed(names):
    return {(site, branch) for n in names for cl in batches()[n]["claims"].values() for site, branch in cl}


def test_the_claims_cover_every_site_and_every_reachable_branch():
    """the 1024-bit list: per site, the add-back at the highest position its operands reach, at a middle one and at 0; an estimate of 2^32
    or more and the break at every site with more than one digit; two loop turns wherever a case key's divisor has v2 >= v1"""
    got = _claimed(NAMES[:6])
    pos = lambda site: sorted(int(b[8:]) for s, b in got if s == site and b.startswith("addback@"))
    assert len(W.SITES) == 14
    for site in W.SITES:
        assert pos(site), site
    for site in ("split_sq_p", "split_sq_q"):                   # nx - nm = 32 (50 under the short q): the top step, the middle, 0
        assert pos(site)[0] == 0 and pos(site)[-1] >= 32 and len(pos(site)) >= 3
    assert 32 in pos("split_sq_p") and 50 in pos("split_sq_q")
    for site in ("split_root_p", "finish_Lh_p", "finish_Lh_q", "crt_m_prod", "crt_r_prod"):     # quotients below the divisor: nm - 1 = 15 is the top
        assert pos(site)[0] == 0 and pos(site)[-1] == 15 and len(pos(site)) >= 3, site
    assert pos("split_root_q")[0] == 0 and len(pos("split_root_q")) >= 3
    for site in ("crt_m_vp", "crt_r_vp"):                       # the short q: 9 and 10 digits; 8 is S31's top step
        assert pos(site)[0] == 0 and pos(site)[-1] == 8 and len(pos(site)) >= 3
    assert pos("key_a0") == [0] and pos("key_a3") == [0] and pos("key_a1") == [3] and pos("key_a2") == [3]
    for site in W.SITES[4:] + ("key_a1", "key_a2"):
        assert (site, "overflow") in got and (site, "break") in got, site
    for site in ("split_sq_q", "split_root_p", "finish_Lh_p", "crt_m_prod", "crt_r_prod", "key_a1", "key_a2"):
        assert (site, "two_turns") in got, site
    # the wide repeats: 2048 bits, every site; 4096 bits, the three the ladder's cost allows
    wide = _claimed(["wide 2048"])
    assert {s for s, b in wide if b.startswith("addback@")} == set(W.SITES)
    assert {s for s, b in _claimed(["wide 4096"]) if b.startswith("addback@")} == {"split_sq_p", "finish_Lh_q", "crt_m_vp"}


def test_the_list_covers_the_lengths_and_shifts():
    """a divisor shorter than a chunk, lengths that are no multiple of it, shift 0 and shift 31 — with the add-back taken there — and a
    first step whose scratch word x[nx] is not zero"""
    seen = set()
    for name in NAMES[:6]:
        b = batches()[name]
        for i in b["crafted"]:
            sites = records(name, i)[1]
            for site, branch in b["claims"][i]:
                if branch.startswith("addback@"):
                    seen.add((site, sites[site]["nm"], sites[site]["s"]))
    lengths = {(nm, s) for _, nm, s in seen}
    assert any(nm < 8 for nm, _ in lengths) and any(nm > 8 and nm % 8 for nm, _ in lengths)
    assert any(s == 0 for _, s in lengths) and any(s == 31 for _, s in lengths) and any(0 < s < 31 for _, s in lengths)
    assert {site for site, nm, s in seen if nm == 7} >= {"split_root_q", "finish_Lh_q", "crt_m_vp", "crt_m_prod", "crt_r_vp", "crt_r_prod"}
    assert {site for site, nm, s in seen if s == 31} >= {"split_root_q", "finish_Lh_q", "crt_m_vp", "crt_m_prod", "crt_r_vp", "crt_r_prod"}
    assert {nm for site, nm, s in seen if site == "split_sq_q"} >= {14, 15, 32}
    b = batches()["split 0"]
    i = b["tag"].index("sq@15 high K1 p")
    assert records("split 0", i)[1]["split_sq_p"]["s"] == 1 and b["c"][i] >> 2047 == 1       # x[nx] = c >> (2048 - s)


def test_the_composite_key_with_a_generic_c_fails_in_the_finish_alone():
    b = batches()["keys 0"]
    i = b["tag"].index("composite p, generic c")
    p, q = _key(b, i)
    got, sites = records("keys 0", i)
    assert not _is_prime(p) and M.key_constants(p, q) is not None
    assert got == (0, 0, 2) == b["want"][i]
    assert set(W.SITES) <= set(sites), "key preparation accepted the key: the item runs to the finish"
    assert not any(st.get("addbacks") for st in sites.values())
    x_p = pow(b["c"][i] % (p * p), p - 1, p * p)
    assert x_p % p != 1 and pow(b["c"][i] % (q * q), q - 1, q * q) % q == 1               # pd_divexact's remainder test, on the p side


def test_divexact_records():
    """the propagation counts of pd_divexact: L = (x_p - 1) / p leaves nothing above word i + nd in most steps, and reaches the top word
    only through a long borrow"""
    st = {}
    q, exact = W.pd_divexact(W.to_words(3 * 5, 4), W.to_words(3, 1), 2, st)
    assert exact and W.from_words(q) == 5 and st == dict(propagation_steps=0, reached_top=False)
    st = {}
    d = (1 << 32) - 1
    x = d * ((1 << 64) - 1)                                     # q_0 d borrows all the way up
    q, exact = W.pd_divexact(W.to_words(x, 3), W.to_words(d, 1), 2, st)
    assert exact and W.from_words(q) == (1 << 64) - 1 and st["propagation_steps"] >= 2 and st["reached_top"]
    _, sites = records("finish 0", 1)
    assert set(sites["divexact_p"]) == {"propagation_steps", "reached_top"}


@pytest.mark.parametrize("name", NAMES)
def test_word_model_definitions_and_upstream_agree(name):
    b = batches()[name]
    rows = range(len(b["c"])) if b["n_bits"] == 1024 else b["crafted"] + [0]
    for i in rows:
        p, q = _key(b, i)
        assert records(name, i)[0] == b["want"][i] == M.open(p, q, b["c"][i]), b["tag"][i]
        if _is_prime(p) and _is_prime(q):
            assert b["want"][i][2] == 0 and M.open_upstream(p, q, b["c"][i]) == b["want"][i][:2], b["tag"][i]
        if b["truth"][i] is not None:
            assert b["want"][i] == (b["truth"][i][0], b["truth"][i][1], 0)
    assert sum(w[2] == 2 for w in b["want"]) == (1 if name == "keys 0" else 0)


@pytest.mark.parametrize("name", NAMES)
def test_every_claimed_item_exposes_its_branch_s_defect(name):
    """the word model with the branch's line removed at the claimed site: other outputs than the truth"""
    b = batches()[name]
    asserted = 0
    for i in b["crafted"]:
        for site, branch in b["claims"][i]:
            fault = FAULT_OF.get(branch.split("@")[0])
            if fault is None or fault in BC.UNOBSERVABLE or (b["tag"][i], site, fault) in BC.UNOBSERVABLE_ITEMS:
                continue
            sites = {}
            got = W.open_words(*_key(b, i), b["c"][i], b["n_bits"] // 64, sites, (site, fault))
            assert sites[site]["derailed"] == 1, (b["tag"][i], site, fault)
            assert got != b["want"][i], (b["tag"][i], site, fault)
            asserted += 1
    assert asserted >= len(b["crafted"]) // 2


def test_no_addback_is_observable_at_every_site():
    seen = set()
    for name in NAMES[:6]:
        b = batches()[name]
        for i in b["crafted"]:
            for site, branch in b["claims"][i]:
                if branch.startswith("addback@") and (b["tag"][i], site, "no_addback") not in BC.UNOBSERVABLE_ITEMS:
                    seen.add(site)
    assert seen == set(W.SITES) and "no_addback" not in BC.UNOBSERVABLE and "no_rh_break" not in BC.UNOBSERVABLE


def test_the_unasserted_faults_are_what_the_table_says():
    """no_overflow_clause: every claimed item gives the true outputs without the clause (the table's reasoning); the listed items too"""
    for name in NAMES[:7]:
        b = batches()[name]
        for i in b["crafted"]:
            for site, branch in b["claims"][i]:
                fault = FAULT_OF.get(branch.split("@")[0])
                if fault == "no_overflow_clause" or (b["tag"][i], site, fault) in BC.UNOBSERVABLE_ITEMS:
                    assert W.open_words(*_key(b, i), b["c"][i], b["n_bits"] // 64, None, (site, fault)) == b["want"][i], (b["tag"][i], site)
    tags = {b["tag"][i] for n in NAMES for b in [batches()[n]] for i in b["crafted"]}
    assert {t for t, _, _ in BC.UNOBSERVABLE_ITEMS} <= tags


def test_faults_leave_ordinary_operands_alone_and_change_the_crafted_ones():
    """pd_mod alone: a fault whose line never runs is the routine itself; on Knuth's example the missing add-back is a wrong remainder"""
    rnd = random.Random(7)
    for _ in range(50):
        x, m = rnd.getrandbits(256), rnd.getrandbits(128) | 1
        st = {}
        for fault in W.FAULTS:
            got = W.pd_mod(W.to_words(x, 8) + [0], 8, W.to_words(m, 4), st, fault)
            assert W.from_words(got) == x % m or st["derailed"]
    u, v = 0x7fffffff_80000000_00000000_00000000, 0x80000000_00000000_00000001
    st = {}
    got = W.pd_mod(W.to_words(u, 4) + [0], 4, W.to_words(v, 3), st, "no_addback")
    assert W.from_words(got) != u % v and st["derailed"] == 1 and st["addback_at"] == [0] and st["s"] == 0 and st["nm"] == 3


def test_random_operands_do_not_reach_the_add_back():
    """200 random 2048-bit ciphertexts modulo p^2 and q^2 of the test key: thousands of digits and corrections, no add-back, no estimate
    of 2^32 — and the break fires for one of the two top words only.  (A fixed seed: this documents, it cannot flake.)"""
    p, q, _ = H.test_key(1024)
    rnd = random.Random(2 ** 31)
    sp, sq = {}, {}
    for _ in range(200):
        c = rnd.getrandbits(2048)
        for F, st in ((p, sp), (q, sq)):
            got = W.pd_mod(W.to_words(c, 64) + [0], 64, W.to_words(F * F, 32), st)
            assert W.from_words(got) == c % (F * F)
    for st in (sp, sq):
        assert st["digits"] == 6600 and st["corrections"] > 1000
        assert st["addbacks"] == 0 and st["overflows"] == 0 and st["addback_at"] == [] and st["max_loops"] <= 2
    assert sp["breaks"] == 0 and sq["breaks"] > 500                         # top words 0x806e.. and 0xe021..


def test_the_crafted_keys_are_inside_the_domain_of_correct_key_prove_too():
    """(tests/ck_prove_model.py needs no change for them: the same domain rules, the CRT formulas applied to the key the caller gave)"""
    import ck_prove_model as CM
    keys = BC.composite_factor_keys() + sorted(BC.prime_keys_with_add_back(16).items())
    assert [name for name, _ in keys] == ["A03", "B12", "C", "P03", "P12"]
    for name, (p, q) in keys:
        assert CM.status(p, q) == 0 and p < 1 << 512 and q < 1 << 512 and (_is_prime(p) and _is_prime(q)) == name.startswith("P"), name
        if name.startswith("P"):
            assert CM.crt(p, q, 12345) == CM.plain(p, q, 12345)


def test_shared_key_and_reversed_batches():
    s = BC.shared_1024()
    assert len(s["keys"]) == 1 and 30 <= len(s["crafted"]) and len(s["c"]) <= 80
    assert all(M.open(*s["keys"][0], c) == w for c, w in zip(s["c"], s["want"]))
    r = BC.reversed_batch(s)
    assert r["c"] == s["c"][::-1] and [r["tag"][i] for i in r["crafted"]] == [s["tag"][i] for i in s["crafted"]][::-1]
    assert any(i % 16 != j % 16 for i, j in zip(s["crafted"], r["crafted"][::-1]))     # the crafted lanes change position within a block
    name, b = BC.list_1024()[0]
    rb = BC.reversed_batch(b)
    assert all(M.open(*rb["keys"][i], rb["c"][i]) == rb["want"][i] for i in rb["crafted"])
