// The host aligner (guacamole_amd/csrc/gq_align_host.h, the body of gq_align_host) as a stand-alone
// program over the tie and edge cases, for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all align_check.cpp
// Prints one line per pair: ref_start ref_end score_int CIGAR.  Exit 0 when every expectation below
// holds.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../guacamole_amd/csrc/gq_align_host.h"

namespace {

struct Case {
  const char *seq, *ref, *cigar;  // cigar: nullptr = not pinned here
};

std::string cigar_of(const gq_alignments *a, int64_t i) {
  static const char ops[] = "MIDNSHP=X";
  std::string s;
  for (int64_t k = a->cigar_off[i]; k < a->cigar_off[i + 1]; ++k)
    s += std::to_string(a->cigar[k] >> 4) + ops[a->cigar[k] & 15];
  return s;
}

}  // namespace

int main() {
  const std::vector<Case> cases = {
      {"TCGA", "TCGA", "4="},
      {"TCGA", "TCCA", "2=1X1="},
      {"TCCGA", "TCGA", "2=1I2="},
      {"TCGACCCTCTGA", "TCGATCTGA", "4=3I5="},
      {"TCGATCTGA", "TCGACCCTCTGA", "4=3D5="},
      {"TCGACCCTCTTA", "TCGATCTGA", "4=3I3=1X1="},
      {"A", "AAAA", "1="},
      {"AAA", "AAAAAAA", "3="},
      {"AAAAAAA", "AAA", nullptr},
      {"ACAC", "ACACAC", "4="},
      {"TCGAGG", "TCGA", "4=2I"},
      {"GGTCGA", "TCGA", "2I4="},
      {"TCGATTTGA", "TCGATTTCGA", "7=1D2="},
      {"ACGTACGTTTTTTTGGGGCCCCGGAACCTTGGCA", "ACGTACGTAAAAAAGGGGCCCCGGAACCTTGGCA", nullptr},
      {"ACGT", "", "4I"},
      {"", "ACGT", ""},
      {"", "", ""},
      {"G", "ACGT", "1="},
      {"G", "ACT", nullptr},
      {"acgt", "ACGT", "4I"},
      {"ATTCTCAAGTTTTAAGTGGTacgtTAACTGAATAAAGAGATTCATCATGTGCAA", "ATTCTCAAGTTTTAAGTGGTACGTTAACTGAATAAAGAGATTCATCATGTGCAA",
       "20=4X30="},
      {"ACNNGT", "TTACNNGTAA", "6="},
  };
  std::vector<uint8_t> seq_pool, ref_pool;
  std::vector<int64_t> seq_off, ref_off;
  std::vector<int32_t> seq_len, ref_len;
  for (const Case &c : cases) {
    seq_off.push_back((int64_t)seq_pool.size());
    ref_off.push_back((int64_t)ref_pool.size());
    seq_len.push_back((int32_t)strlen(c.seq));
    ref_len.push_back((int32_t)strlen(c.ref));
    seq_pool.insert(seq_pool.end(), c.seq, c.seq + strlen(c.seq));
    ref_pool.insert(ref_pool.end(), c.ref, c.ref + strlen(c.ref));
  }
  // exact-size heap copies, so that a read past a pool's end is caught
  std::vector<uint8_t> sp(seq_pool.begin(), seq_pool.end()), rp(ref_pool.begin(), ref_pool.end());
  sp.shrink_to_fit();
  rp.shrink_to_fit();
  gq_align_params p;
  memset(&p, 0, sizeof(p));
  p.mismatch_probability = std::exp(-4.0);
  p.open_gap_probability = std::exp(-6.0);
  p.close_gap_probability = 1 - std::exp(-1.0);
  if (!gq_align::valid(p)) return 2;
  double t[32];
  gq_align::penalty_table(p, t);
  gq_alignments *a = nullptr;
  int64_t bad = -1;
  if (gq_align::align_host((int64_t)cases.size(), sp.data(), seq_off.data(), seq_len.data(), rp.data(), ref_off.data(),
                           ref_len.data(), t, &a, &bad))
    return 2;
  int wrong = 0;
  for (size_t i = 0; i < cases.size(); ++i) {
    const std::string got = cigar_of(a, (int64_t)i);
    printf("%d %d %d %s\n", a->ref_start[i], a->ref_end[i], a->score_int[i], got.c_str());
    if (cases[i].cigar && got != cases[i].cigar) {
      fprintf(stderr, "case %zu: CIGAR %s, expected %s\n", i, got.c_str(), cases[i].cigar);
      ++wrong;
    }
  }
  if (a->ref_end[6] != 1) {
    fprintf(stderr, "A in AAAA ends at %d, expected 1\n", a->ref_end[6]);
    ++wrong;
  }
  gq_align::free_block(a);
  return wrong ? 1 : 0;
}
