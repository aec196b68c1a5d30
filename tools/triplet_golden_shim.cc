// triplet_golden_shim.cc -- drives the reference's own FST builders (src/lib/mutation_fst.cc, compiled from the
// reference tree by tools/make_golden_triplet.py; nothing of it is in this repository) through OpenFst, to record
// what the reference's FST aligner answers.  The two coati symbols mutation_fst.o needs from elsewhere come from here:
//   coati::mg94_p            returns the 61x61 P the generator computed with THIS project's host model (a file), so the
//                            fixtures pin the alignment algorithm, not the matrix exponential
//   coati::utils::get_nuc    nucleotide `pos` of sense codon `cod` in AAA..TTT order without the stops
//
// stdin, one job per line:
//   align <codon|dna> <P file> <gap_open> <gap_extend> <bc_error> <pi A C G T> <ancestor> <descendant>
//     -> "<score %.9g> <aligned ancestor> <aligned descendant>"   ("-" for an empty sequence)
//   checks <P file>  -> the arc / state counts and dna arc weights the reference's doctests check
// (sequences as the aligner sees them: validated, end stops already trimmed)
#include <fst/fstlib.h>

#include <coati/dna_syms.hpp>
#include <coati/mutation_coati.hpp>
#include <coati/mutation_fst.hpp>
#include <coati/utils.hpp>

#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

namespace {
std::vector<float> g_P(61 * 61);
std::map<std::string, std::vector<float>> g_cache;

void load_P(const std::string& path) {
    auto it = g_cache.find(path);
    if(it == g_cache.end()) {
        std::ifstream in(path, std::ios::binary);
        std::vector<float> P(61 * 61);
        in.read(reinterpret_cast<char*>(P.data()), sizeof(float) * P.size());
        if(!in) throw std::runtime_error("cannot read " + path);
        it = g_cache.emplace(path, std::move(P)).first;
    }
    g_P = it->second;
}

const int kSense[61] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20,
                        21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41,
                        42, 43, 44, 45, 46, 47, 49, 51, 52, 53, 54, 55, 57, 58, 59, 60, 61, 62, 63};
}  // namespace

namespace coati {
Matrixf mg94_p(float_t, float_t, const std::vector<float_t>&, const std::vector<float_t>&) {
    return Matrixf(61, 61, g_P.begin(), g_P.end());
}
namespace utils {
uint8_t get_nuc(uint8_t cod, int pos) { return static_cast<uint8_t>((kSense[cod] >> (2 * (2 - pos))) & 3); }
}  // namespace utils
}  // namespace coati

namespace {
using fst::StdArc;
using coati::VectorFstStdArc;

// align_fst.cc's sequence of OpenFst calls: evolution = optimize(mutation o indel) without epsilons, then
// ancestor o evolution o descendant, ShortestPath, ShortestDistance, TopSort
void align(const std::string& kind, float g, float e, float b, const std::vector<float>& pi, const std::string& anc,
           const std::string& des) {
    VectorFstStdArc mut = kind == "codon" ? coati::mg94(0.0133f, 0.2f, pi) : coati::dna(0.0133f, 0.2f, pi);
    VectorFstStdArc ind = coati::indel(g, e, pi, b);
    VectorFstStdArc mut_sort(fst::ArcSortFst<StdArc, fst::OLabelCompare<StdArc>>(mut, fst::OLabelCompare<StdArc>()));
    VectorFstStdArc ind_sort(fst::ArcSortFst<StdArc, fst::ILabelCompare<StdArc>>(ind, fst::ILabelCompare<StdArc>()));
    VectorFstStdArc tmp = VectorFstStdArc(fst::ComposeFst<StdArc>(mut_sort, ind_sort));
    VectorFstStdArc evo_opt = coati::optimize(tmp);
    VectorFstStdArc evo{fst::RmEpsilonFst<StdArc>(evo_opt)};
    VectorFstStdArc fa, fb;
    coati::acceptor(anc, fa);
    coati::acceptor(des, fb);
    fst::ComposeFst<StdArc> inter(fa, evo);
    VectorFstStdArc inter_sort(fst::ArcSortFst<StdArc, fst::OLabelCompare<StdArc>>(inter, fst::OLabelCompare<StdArc>()));
    VectorFstStdArc graph;
    fst::Compose(inter_sort, fb, &graph);
    VectorFstStdArc path;
    fst::ShortestPath(graph, &path);
    std::vector<StdArc::Weight> dist;
    fst::ShortestDistance(path, &dist);
    fst::TopSort(&path);
    static const char* sym = "-ACGTN";
    std::string s1, s2;
    fst::StateIterator<fst::StdFst> it(path);
    for(int i = 0; i < path.NumStates() - 1; it.Next(), ++i) {
        fst::ArcIteratorData<StdArc> arcs;
        path.InitArcIterator(it.Value(), &arcs);
        s1.push_back(sym[arcs.arcs[0].ilabel]);
        s2.push_back(sym[arcs.arcs[0].olabel]);
    }
    std::printf("%.9g %s %s\n", dist.empty() ? -1.0 : static_cast<double>(dist[0].Value()), s1.empty() ? "-" : s1.c_str(),
                s2.empty() ? "-" : s2.c_str());
}

void checks() {
    const std::vector<float> pi{0.308f, 0.185f, 0.199f, 0.308f};
    VectorFstStdArc mg = coati::mg94(0.0133f, 0.2f, pi);
    VectorFstStdArc d = coati::dna(0.0133f, 0.2f, pi);
    VectorFstStdArc ind = coati::indel(0.001f, 1.f - 1.f / 6.f, pi, 0.0001f);
    std::printf("mg94_arcs0 %zu\ndna_arcs0 %zu\ndna_states %d\nindel_states %d\n", mg.NumArcs(0), d.NumArcs(0), d.NumStates(),
                ind.NumStates());
    for(int s = 0; s < ind.NumStates(); ++s) std::printf("indel_arcs%d %zu\n", s, ind.NumArcs(s));
    fst::ArcIteratorData<StdArc> arcs;
    d.InitArcIterator(0, &arcs);
    std::printf("dna_weights");
    for(size_t i = 0; i < arcs.narcs; ++i) std::printf(" %d:%d:%.9g", arcs.arcs[i].ilabel, arcs.arcs[i].olabel, arcs.arcs[i].weight.Value());
    std::printf("\n");
}
}  // namespace

int main() {
    std::string line;
    while(std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        in >> op;
        if(op == "align") {
            std::string kind, path, anc, des;
            float g, e, b;
            std::vector<float> pi(4);
            in >> kind >> path >> g >> e >> b >> pi[0] >> pi[1] >> pi[2] >> pi[3] >> anc >> des;
            if(anc == "-") anc.clear();
            if(des == "-") des.clear();
            load_P(path);
            align(kind, g, e, b, pi, anc, des);
        } else if(op == "checks") {
            std::string path;
            in >> path;
            load_P(path);
            checks();
        }
        std::fflush(stdout);
    }
    return 0;
}
