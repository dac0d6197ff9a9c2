"""A Python restatement of the library's routing of RangeProofNi calls under ONE 2048-bit key (zk-paillier_amd/csrc/route_plan.hpp), as a
function of the compute units and of the secondary engines that are loaded: tests/test_gpu_routing.py compares it with what ran on the
device, tests/test_cpp_route_plan.py with the header itself at every batch size, on a CPU."""


def expected_family(cus, lat, mid, items, listed=False):
    """what the library is expected to pick for a Paillier launch of `items` Enc under ONE 2048-bit key that the base-n form takes
    (route_engine with one_key_paillier, basen_plan of either engine).  lat / mid: limbs per lane of the latency / mid engine (0: not loaded).
    listed: `items` is the bound of a verify's work list — three quarters of it (+ 3 %) are expected to exist, and the mid engine's
    one-round window is judged by that (route_plan.hpp expected_items)"""
    simds = 4 * cus
    one_round = items <= 16 * simds or (listed and (3 * items + 3) // 4 + items // 32 <= 16 * simds)
    lat_round = listed and (3 * items + 3) // 4 + items // 32 <= 8 * simds      # a verify that fits one round of the latency engine's k_enc_basen<8>
    if lat == 9 and mid == 18 and ((16 * simds < items <= 24 * simds and not one_round) or 4 * simds < items <= 5 * simds or (8 * simds < items <= 9 * simds and not lat_round)
                                  or (not listed and 32 * simds < items <= 40 * simds)):
        return "split"                                         # two concurrent calls (expected_tail below)
    if mid == 18 and ((10 * simds < items and one_round) or 32 * simds < items <= 48 * simds):
        return "mid-basen"                                     # 16 Enc per wavefront: one (two) wavefronts per SIMD of the mid engine
    if lat == 9 and items <= 3 * simds * 8:                    # the latency engine: up to three wavefronts per SIMD at 8 Enc per wavefront
        if (min(items, (3 * items + 3) // 4 + items // 32) if listed else items) <= 2 * simds:
            return "lat-r2l"                                   # one Enc per wavefront, the five-group ladder (kernels_basen_r2l.hpp); a verify by its expected items (9, 10 proofs)
        return "lat-basen" if items > simds * 4 else "lat-n2"
    return "base-n" if items > simds * 16 else "n2"


def expected_tail(cus, B):
    """proofs of a split call that run on the second latency-engine ctx (route_plan.hpp: range_split; 256 Enc per proof)"""
    simds = 4 * cus
    full, least = 16 * simds // 256, 4 * simds // 256
    if B * 256 <= 5 * simds:
        return B - least                                       # 17 ... 20 proofs: 16 on the window ladder, the rest on the one-Enc-per-wavefront ladder
    if B * 256 <= 9 * simds:
        return B - 8 * simds // 256                            # 33 ... 36 proofs (prove): 32 on k_enc_basen<8>, the rest on the one-Enc-per-wavefront ladder
    if B * 256 > 32 * simds:
        t = B - 32 * simds // 256                              # 129 ... 160 proofs (prove): 128 on the throughput engine, the rest beside them on the latency engine
        return 2 * simds // 256 + 1 if 3 * simds // 2 < t * 256 <= 2 * simds else t      # (not 7 or 8 proofs: the r2l ladder's workgroups would not fit beside the head)
    return B - full if B - full >= least else least            # 65 ... 96: 64 on the mid engine | at least 16 on the latency engine


def expected_family_throughput(cus, items):
    return "base-n" if items > 4 * cus * 16 else "n2"
