// The triplet models (tri-mg, tri-ecm, dna): the reference's FST aligner, with the shortest path computed
// by a DP on the GPU (coati_hip_triplet_align, include/coati_hip.h) instead of by OpenFst composition.
//
// Mirrors (same names, argument meaning and errors):
//   fst_alignment                        src/lib/align_fst.cc:46-110
//   process_triplet                      src/lib/utils.cc:1102-1135
//   set_subst (triplet branches)         src/lib/utils.cc:609-616
//   mg94 / dna / ecm arc weights         src/lib/mutation_fst.cc, mutation_ecm.cc:194-218
// Extension: fst_alignment_batch -- consecutive pairs, one launch, a JSON array out.
#ifndef COATI_AMD_HOST_TRIPLET_HPP
#define COATI_AMD_HOST_TRIPLET_HPP

#include <array>
#include <string>
#include <vector>

#include "align.hpp"

namespace coati_amd {

// What coati_hip_triplet_model_create takes for a model: the substitution weights and the pi indel() sees.
struct triplet_model_t {
    bool codon{true};         // tri-mg, tri-ecm: 61x61; dna: 4x4
    std::vector<float> cost;  // add_arc weights: -logf(P) (0 where P == 1, INT_MAX where P == 0)
    std::array<float, 4> pi;  // tri-ecm: the ECM frequencies (set_subst overrides aln.pi)
};

bool is_triplet_model(const std::string& model);
// set_subst's triplet branches; throws std::invalid_argument("Mutation model unknown.") for any other model.
// tri-mg uses aln.sigma as mar-mg does here; dna uses mg94_p without sigma, as dna() does.
triplet_model_t triplet_model(const alignment_t& aln);
// dna()'s 4x4 dna_p (normalised rows), before add_arc
std::array<float, 16> dna_p(const matrix61_t& P);

// process_triplet: exactly two sequences, -r / -v ordering, ancestor a whole number of codons without an early
// stop or an ambiguous nucleotide; descendant only ACGTUN (either case); end stops trimmed into data.stops.
void process_triplet(data_t& data, const std::string& refs, bool rev);

bool fst_alignment(alignment_t& aln);
bool fst_alignment_batch(alignment_t& aln);

}  // namespace coati_amd
#endif
