// The host-composition route of tools/dev/ck_inter_ab.py: CorrectKey::challenge and CorrectKey::prove (host/zkproofs.hpp), once per session,
// against challenge_batch_seeded / prove_batch / verify_batch_seeded over the same keys.  Reads "p q" in decimal, one key per line, from the
// file named on the command line; prints one JSON object.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../zk-paillier_amd/host/zkproofs.hpp"

using namespace zkproofs;

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s KEYS_FILE\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  std::vector<DecryptionKey> keys;
  std::string p, q;
  while (in >> p >> q) keys.push_back(DecryptionKey{BigInt::from_str_radix10(p), BigInt::from_str_radix10(q)});
  if (keys.empty()) { std::fprintf(stderr, "no keys\n"); return 2; }
  try {
    std::vector<const DecryptionKey*> ptrs;
    std::vector<EncryptionKey> eks;
    for (const DecryptionKey& k : keys) { ptrs.push_back(&k); const BigInt n = k.p * k.q; eks.push_back(EncryptionKey{n, n * n}); }
    const CorrectKey::VerifierSeed seed = CorrectKey::VerifierSeed::fresh();
    (void)CorrectKey::prove(keys[0], CorrectKey::challenge(eks[0]).first);      // warm-up of both routes
    (void)CorrectKey::prove_batch(ptrs, CorrectKey::challenge_batch_seeded(eks, seed, 0));
    std::vector<Challenge> ch;
    StopWatch sw;
    for (const EncryptionKey& ek : eks) ch.push_back(CorrectKey::challenge(ek).first);
    const double chal_ms = sw.lap();
    bool ok = true;
    for (size_t k = 0; k < keys.size(); k++) ok = CorrectKey::prove(keys[k], ch[k]).is_ok() && ok;
    const double prove_ms = sw.lap();
    const std::vector<Challenge> bch = CorrectKey::challenge_batch_seeded(eks, seed, 1);
    const double bchal_ms = sw.lap();
    const std::vector<CorrectKey::ProveResult> res = CorrectKey::prove_batch(ptrs, bch);
    const double bprove_ms = sw.lap();
    std::vector<CorrectKeyProof> proofs;
    for (const CorrectKey::ProveResult& r : res) { ok = ok && r.is_ok(); proofs.push_back(r.ok ? r.proof : CorrectKeyProof{}); }
    for (const Result& r : CorrectKey::verify_batch_seeded(eks, seed, 1, proofs)) ok = ok && r.is_ok();
    const double bverify_ms = sw.lap();
    std::printf("{\"sessions\": %zu, \"challenge_per_session_ms\": %.3f, \"prove_per_session_ms\": %.3f, \"challenge_batch_seeded_ms\": %.3f, "
                "\"prove_batch_ms\": %.3f, \"verify_batch_seeded_ms\": %.3f, \"all_accept\": %s}\n",
                keys.size(), chal_ms / keys.size(), prove_ms / keys.size(), bchal_ms, bprove_ms, bverify_ms, ok ? "true" : "false");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "failed: %s\n", e.what());
    return 1;
  }
}
