"""A Python restatement of the library's routing of RangeProofNi calls under ONE 2048-bit key (zk-paillier_amd/csrc/route_plan.hpp), as a
function of the compute units and of the secondary engines that are loaded: tests/test_gpu_routing.py and
tests/test_gpu_range_error_factors.py compare it with what ran on the device, tests/test_cpp_route_plan.py with the header itself at every
batch size and at six row counts, on a CPU."""


def expected_items(bound):
    """the items a verify's work list is expected to hold when 2 per row are its bound: three quarters, + 3 %"""
    return (3 * bound + 3) // 4 + bound // 32


def expected_split(cus, B, rows_per_proof=256, listed=False):
    """(head, engine of the head: "mid" | "lat" | "own", items per SIMD of the round the head has to fit) of a call of B proofs at rows_per_proof Enc per proof (2 per row) that runs as two
    concurrent calls — the first `head` proofs there, the rest on a second ctx of the latency engine — or None (route_plan.hpp: range_split,
    both secondary engines loaded).  Every window is one of ITEMS; a head is the whole proofs that fit the engine's one round."""
    simds = 4 * cus
    items = B * rows_per_proof
    if rows_per_proof == 0:
        return None
    if listed and items > 16 * simds and expected_items(items) <= 16 * simds:
        return None                                            # a verify the mid engine takes in one round by its expected items
    if 16 * simds < items <= 24 * simds:
        # 65 ... 96 proofs at 256 per proof: one round of the mid engine | at least one round of the latency engine's window ladder
        full, least = 16 * simds // rows_per_proof, 4 * simds // rows_per_proof
        head, engine, per_simd = (full if B - full >= least else max(B - least, 0)), "mid", 16
    elif 8 * simds < items <= 9 * simds and not (listed and expected_items(items) <= 8 * simds):
        head, engine, per_simd = 8 * simds // rows_per_proof, "lat", 8      # 33 ... 36 proofs (prove): 32 on k_enc_basen<8>, the rest on the one-Enc-per-wavefront ladder
    elif not listed and 32 * simds < items <= 40 * simds:
        head, engine, per_simd = 32 * simds // rows_per_proof, "own", 32     # 129 ... 160 proofs (prove): 128 on the throughput engine, the rest beside them on the latency engine
        if 3 * simds // 2 < (B - head) * rows_per_proof <= 2 * simds:
            head = B - (2 * simds // rows_per_proof + 1)       # (not 7 or 8 proofs: the r2l ladder's workgroups would not fit beside the head)
    elif 4 * simds < items <= 5 * simds:
        head, engine, per_simd = 4 * simds // rows_per_proof, "lat", 4      # 17 ... 20 proofs: 16 on the window ladder, the rest on the one-Enc-per-wavefront ladder
    else:
        return None
    return (head, engine, per_simd) if 0 < head < B else None


def expected_family(cus, lat, mid, items, listed=False, rows_per_proof=256, never_split=False):
    """what the library is expected to pick for a Paillier launch of `items` Enc under ONE 2048-bit key that the base-n form takes
    (route_engine with one_key_paillier, basen_plan of either engine).  lat / mid: limbs per lane of the latency / mid engine (0: not loaded).
    listed: `items` is the bound of a verify's work list — three quarters of it (+ 3 %) are expected to exist, and the mid engine's
    one-round window is judged by that (route_plan.hpp expected_items).
    rows_per_proof: Enc per proof (2 per row) of the RangeProofNi call the items belong to — a split cuts between proofs.
    never_split: the caller does not ask range_split — zkp_range_ni_prove_batch with an error factor other than 128 in the struct, and the
    three interactive entry points (generate_encrypted_pairs, the prove of any other row count, among them)"""
    simds = 4 * cus
    one_round = items <= 16 * simds or (listed and expected_items(items) <= 16 * simds)
    if (not never_split and lat == 9 and mid == 18 and rows_per_proof and items % rows_per_proof == 0
            and expected_split(cus, items // rows_per_proof, rows_per_proof, listed)):
        return "split"                                         # two concurrent calls (expected_tail below)
    if mid == 18 and ((10 * simds < items and one_round) or 32 * simds < items <= 48 * simds):
        return "mid-basen"                                     # 16 Enc per wavefront: one (two) wavefronts per SIMD of the mid engine
    if lat == 9 and items <= 3 * simds * 8:                    # the latency engine: up to three wavefronts per SIMD at 8 Enc per wavefront
        if (min(items, expected_items(items)) if listed else items) <= 2 * simds:
            return "lat-r2l"                                   # one Enc per wavefront, the five-group ladder (kernels_basen_r2l.hpp); a verify by its expected items (9, 10 proofs)
        return "lat-basen" if items > simds * 4 else "lat-n2"
    return "base-n" if items > simds * 16 else "n2"


def expected_tail(cus, B, rows_per_proof=256, listed=False):
    """proofs of a split call that run on the second latency-engine ctx (route_plan.hpp: range_split; 256 Enc per proof at 128 rows); 0: the
    call is not cut.  (At 256 per proof the windows of a prove and of a verify that is cut give the same tail: `listed` only decides
    WHETHER — expected_family says that.)"""
    cut = expected_split(cus, B, rows_per_proof, listed)
    return B - cut[0] if cut else 0


def expected_family_throughput(cus, items):
    return "base-n" if items > 4 * cus * 16 else "n2"
