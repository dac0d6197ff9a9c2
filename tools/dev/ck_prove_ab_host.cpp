// Measurement (C) of tools/dev/ck_prove_ab.py: the host API's single-key NiCorrectKeyProof::proof, once per key, against proof_batch over
// the same keys.  Reads "p q" in decimal, one key per line, from the file named on the command line; prints one JSON object.
#include <chrono>
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
    for (const DecryptionKey& k : keys) ptrs.push_back(&k);
    (void)NiCorrectKeyProof::proof(keys[0]);                                   // warm-up of both routes
    (void)NiCorrectKeyProof::proof_batch(ptrs);
    std::vector<NiCorrectKeyProof> one;
    StopWatch sw;
    for (const DecryptionKey& k : keys) one.push_back(NiCorrectKeyProof::proof(k));
    const double single_ms = sw.lap();
    const std::vector<NiCorrectKeyProof> all = NiCorrectKeyProof::proof_batch(ptrs);
    const double batch_ms = sw.lap();
    bool same = all.size() == one.size();
    for (size_t k = 0; same && k < one.size(); k++) same = all[k].sigma_vec == one[k].sigma_vec;
    std::printf("{\"keys\": %zu, \"proof_per_key_total_ms\": %.3f, \"proof_ms_per_key\": %.3f, \"proof_batch_ms\": %.3f, \"same\": %s}\n", keys.size(), single_ms,
                single_ms / keys.size(), batch_ms, same ? "true" : "false");
    return same ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "failed: %s\n", e.what());
    return 1;
  }
}
