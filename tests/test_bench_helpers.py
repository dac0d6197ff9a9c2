"""CPU tests of the bench plumbing that does not need a GPU: the synthetic key material, the algorithmic-work figures of SURVEY.md
§8(d), the PMC file lookup behind `roofline.traffic`."""
import importlib
import math
import os
import sys

import helpers as H

sys.path.insert(0, H.ROOT)
import bench  # noqa: E402

synth = importlib.import_module("zk-paillier_amd.synth")


def test_bench_key_material():
    p, q, n = synth.bench_key_4096()
    assert n == p * q and n.bit_length() == 4096 and p != q
    assert H.is_probable_prime(p, rounds=4) and H.is_probable_prime(q, rounds=4)
    keys = synth.distinct_keys_2048(4096)
    assert len(set(keys)) == 4096 and all(k.bit_length() == 2048 and k % 2 == 1 for k in keys)
    assert math.gcd(keys[0], keys[1]) > 1 or math.gcd(keys[0], keys[2]) > 1        # products of POOLED primes: neighbours share a factor
    assert synth.BENCH_N == H.fixture_key()[2]


def test_algorithmic_work_figures_match_the_survey():
    # Enc(k=2048) = 8.085e7, Enc(k=4096) = 6.455e8, sigma^n mod n (k=2048) = 2.029e7 limb-MACs
    assert abs(bench.enc_limb_macs(2048) / 8.085e7 - 1) < 1e-3
    assert abs(bench.enc_limb_macs(4096) / 6.455e8 - 1) < 1e-3
    assert abs(bench.modexp_limb_macs(2048, 2048) / 2.029e7 - 1) < 1e-3


def test_pmc_lookup_reads_the_committed_profiles():
    for kernel in ("k_enc<4, true>", "k_enc<4, false>", "k_enc<8, true>", "k_ck_check<2>"):
        per, src = bench.pmc_traffic_per_modexp(kernel)
        assert per and per > 1e4 and os.path.exists(os.path.join(H.ROOT, src)), kernel
    assert bench.pmc_traffic_per_modexp("k_no_such_kernel") == (None, None)


def test_argument_defaults_are_the_baseline_sizes():
    a = bench.parse_args([])
    assert (a.gpus, a.batch, a.n_bits, a.big_batch, a.distinct_batch) == (1, 4096, 2048, 4096, 4096)
    assert not a.full and a.dump_outputs is None             # a plain run: the headline legs only, nothing written


def test_executed_work_figure_follows_the_kernel_script():
    """bench.sliding_ladder_products mirrors k_sliding_schedule (csrc/kernels_modexp.hpp): squarings and other products of the
    fixture key's ladder; the executed multiply-adds per Enc are below the algorithmic 8.085e7 (squarings at 3/4)"""
    def sched(n, swin=6):                      # the device routine, bit for bit
        bit = lambda i: (n >> i) & 1
        sq, mul, i, started = 0, 32, n.bit_length() - 1, False
        while i >= 0:
            if not bit(i):
                sq += 1; i -= 1; continue
            l = max(i - swin + 1, 0)
            while not bit(l):
                l += 1
            if started:
                sq += i - l + 1; mul += 1
            started = True
            i = l - 1
        return sq, mul
    for n in (synth.BENCH_N, synth.bench_key_4096()[2], 1, 0b1000001, (1 << 77) - 1):
        assert bench.sliding_ladder_products(n) == sched(n), n
    ex = bench.executed_lane_mads_per_enc(synth.BENCH_N, 2048, True)
    assert 7.7e7 < ex < 7.9e7 < bench.enc_limb_macs(2048)
    # the roofline is 16 lanes/clk/SIMD: a fraction above 1 is impossible by construction, and the record keeps its factors
    assert bench.PEAK_LIMB_MAC_PER_S == 16 * 1024 * 2.4e9 == bench.valu_mad_peak()
    clock = {"mean_ghz": 2.303, "mean_power_w": 1362.0}
    pmc = {"simd_cycles_per_valu_instr": 4.0033, "valu_wave_instr_per_wave_modexp": 22261665.6, "modexps_per_wavefront": 16}
    r = bench.valu_roofline(34.44e12, 33.19e12, clock, pmc, ex * 16 / 64.0)
    assert r["frac"] < r["frac_at_sampled_clock"] < 1 and abs(r["frac"] - 0.876) < 0.002
    assert abs(r["valu_issue_busy"] * r["mad_share_of_valu"] - r["mad_issue_frac_at_sampled_clock"]) < 0.01
    assert abs(r["frac_at_sampled_clock"] - r["mad_issue_frac_at_sampled_clock"] / r["executed_over_algorithmic"]) < 1e-9


def test_base_n_work_model_and_its_roofline_identity():
    """the work model of the form that ran: 2 / 3 n-sized modular products per squaring / product — 0.544 of SURVEY 8(d)'s
    figure —, the executed count of the base-n kernels, and the identity of the evidence line of round 4 (profiles/bench_r04_basen.json with
    profiles/r04_pmc_basen_enc2048_shared_b4096.json)"""
    assert abs(bench.enc_limb_macs_basen(2048) / 4.396e7 - 1) < 1e-3
    assert abs(bench.enc_limb_macs_basen(2048) / bench.enc_limb_macs(2048) - 0.5438) < 1e-3
    assert abs(bench.enc_limb_macs_basen(4096) / 3.503e8 - 1) < 1e-3
    ex = bench.executed_lane_mads_per_enc_basen(synth.BENCH_N, 2048, engine=False)      # the compiled bodies (rounds 4 - 5; -DZKP_BN_ASM=0)
    sq, mul = bench.sliding_ladder_products(synth.BENCH_N)
    # a squaring: 72 sub-steps x 2 lanes x (54.5 + 72) multiply-adds + 72 for the b side's columns; a product: three n-sized products
    assert ex == sq * (72 * 2 * 126.5 + 72) + mul * (3 * 72 * 2 * 72.0 + 72) + 5 * 72 * 2 * 72.0 + 2 * 72
    assert 4.7e7 < ex < 4.8e7 and ex < bench.executed_lane_mads_per_enc(synth.BENCH_N, 2048, True) * 0.62
    # the assembler engine (round 6): the cross product of a base-n product without a reduction — 2.5 n-sized products per product
    eng = bench.executed_lane_mads_per_enc_basen(synth.BENCH_N, 2048)
    assert eng == ex - (mul + 1) * (0.5 * 72 * 2 * 72.0 - 72) and 0.96 < eng / ex < 0.97
    # ... which is what the lane model counts when it EXECUTES the generated instructions (tests/test_bn_asm.py; a wave instruction is
    # 64 lanes = 32 Enc x 2 lanes): 2 x (1962 + 2592) + 36 multiply-add instructions per squaring, 5 x 2 x 1296 + 72 per product
    assert 72 * 2 * 126.5 + 72 == 2 * (2 * (1962 + 2592) + 36) and 2.5 * 72 * 2 * 72.0 + 2 * 72 == 2 * (5 * 2 * 1296 + 72)
    for kernel in ("k_enc_basen<2>", "k_enc_basen<4>"):
        per, src = bench.pmc_traffic_per_modexp(kernel)
        assert per and per > 1e5 and os.path.exists(os.path.join(H.ROOT, src)), kernel
    rec, _ = bench.pmc_record("k_enc_basen<2>")          # the newest record: what a bench line of today is priced with
    assert rec["_derived"]["modexps_per_wavefront"] == 32 and 4.0 <= rec["_derived"]["simd_cycles_per_valu_instr"] < 4.4
    import json
    # the identity on the evidence of ONE round: round 4's line with round 4's counters (the compiled bodies: engine=False above)
    r04 = json.load(open(os.path.join(H.ROOT, "profiles", "r04_pmc_basen_enc2048_shared_b4096.json")))
    der = next(v["_derived"] for k, v in r04.items() if "k_enc_basen<2>" in k)
    line = json.loads(open(os.path.join(H.ROOT, "profiles", "bench_r04_basen.json")).read().strip().splitlines()[-1])
    r = line["roofline"]
    assert r["work_model"]["form"].startswith("base-n") and r["frac"] < r["frac_at_sampled_clock"] < 1
    assert r["work_model"]["achieved_by_the_survey_8d_model_tlimb_mac_per_s"] > r["peak"]          # the schoolbook model would read above the ceiling
    busy, share = 4.0 / der["simd_cycles_per_valu_instr"], ex * 32 / 64.0 / der["valu_wave_instr_per_wave_modexp"]
    assert abs(busy * share / r["executed_over_algorithmic"] - r["frac_at_sampled_clock"]) < 0.03   # (PMC pass and timed steps ran at slightly different clocks)
    # ... and on round 6's, once it is recorded: the engine's executed count with the engine's counters
    f6 = os.path.join(H.ROOT, "profiles", "bench_r06_final.json")
    if os.path.exists(f6):
        r6 = json.loads(open(f6).read().strip().splitlines()[-1])["roofline"]
        p6 = json.load(open(os.path.join(H.ROOT, "profiles", "r06_pmc_final_enc2048_shared_b4096.json")))
        d6 = next(v["_derived"] for k, v in p6.items() if "k_enc_basen<2>" in k)
        busy6, share6 = 4.0 / d6["simd_cycles_per_valu_instr"], eng * 32 / 64.0 / d6["valu_wave_instr_per_wave_modexp"]
        assert abs(r6["executed_lane_mads_per_enc"] - eng) < 1 and 0.87 < share6 < 0.90
        # (the PMC pass ran on another board, alone; the timed verify launch shares the chip with the transcript hash of its call since
        # the two-stream rule of round 6: the identity holds to 4 % here, to 3 % on round 4's single-stream evidence)
        assert abs(busy6 * share6 / r6["executed_over_algorithmic"] - r6["frac_at_sampled_clock"]) < 0.04
