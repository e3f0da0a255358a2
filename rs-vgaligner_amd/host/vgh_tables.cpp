// vgh_tables.cpp -- the analysis tables of map_reads / map_reads_multi (vgh_tables.hpp): reading them from a context, adding them
// over the contexts, the two rankings and the TSV files.  Nothing of this is in the reference.
#include "vgh_tables.hpp"
#include "../csrc/vga_deletion.hpp"
#include "../csrc/vga_insertion.hpp"
#include "../csrc/vga_pair_index.hpp"
#include "../csrc/vga_phase.hpp"
#include "../csrc/vga_hapcall.hpp"
#include "../csrc/vga_phase_join.hpp"
#include "../csrc/vga_hap_paths.hpp"
#include "../csrc/vga_abundance.hpp"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <fstream>

namespace vgh {

void write_file(const std::string &name, const std::string &body)
{
    std::ofstream o(name, std::ios::binary);
    if (!o) throw Error("Couldn't create file " + name);
    o.write(body.data(), body.size());
    if (!o) throw Error("Couldn't write to file " + name);
}

void Counters::add(const Counters &o)
{
    if (v.size() < o.v.size()) v.resize(o.v.size());
    for (size_t k = 0; k < o.v.size(); k++) {
        if (v[k].size() < o.v[k].size()) v[k].resize(o.v[k].size(), 0);
        for (size_t i = 0; i < o.v[k].size(); i++) v[k][i] += o.v[k][i];
    }
    n[0] += o.n[0];
    n[1] += o.n[1];
}

void Counters::pad(const std::vector<size_t> &sizes)
{
    if (v.size() < sizes.size()) v.resize(sizes.size());
    for (size_t k = 0; k < sizes.size(); k++)
        if (v[k].size() < sizes[k]) v[k].resize(sizes[k], 0);
}

void PhaseStore::add(const PhaseStore &o)
{
    if (words.size() + o.words.size() > PH_MAX_WORDS) throw Error("--phase: the stores of the contexts hold more than 2^32 - 1 words together");
    const uint32_t shift = (uint32_t)words.size();
    for (size_t i = 0; i < o.recs.size(); i++) recs.push_back(o.recs[i] + (i % 3 == 0 ? shift : 0u));
    words.insert(words.end(), o.words.begin(), o.words.end());
}

void PhaseLinks::chain(uint32_t min_links)
{
    const size_t n = pos.size();
    ps.assign(n + 1, 0); flip.assign(n + 1, 0); link_d.assign(n + 1, 0);
    ph_chain(n, links.data(), min_links, ps.data(), flip.data(), link_d.data());
}

bool scoring_on(const MapOptions &opt) { return opt.path_support || opt.genotype || opt.genotype_likelihood || opt.path_edit || opt.haplotype_paths || opt.path_abundance; }

namespace {

bool variant_params_ok(const MapOptions &opt) { return opt.call_error >= 257 && opt.call_error <= 8192 && opt.call_min_depth >= 1; }
bool likelihood_params_ok(const MapOptions &opt) { return opt.genotype_lambda >= 1 && opt.genotype_lambda <= 4096 && opt.genotype_cap >= 1 && opt.genotype_cap <= 255; }

void check(vga_ctx *ctx, int rc)
{
    if (rc != VGA_OK) throw Error(vga_last_error(ctx));
}

// the first n of the library's 32-bit counters as one vector of a table
std::vector<uint64_t> widen(const std::vector<uint32_t> &t, size_t n) { return std::vector<uint64_t>(t.begin(), t.begin() + (long)n); }

// `call(cap, arrays..)` is one of the two library calls with everything before cap bound: asked again when the first answer holds
// more calls than it had room for
template <typename F>
void variant_fetch(vga_ctx *ctx, VariantCalls &v, F call)
{
    uint64_t cap = 4096;
    for (;;) {
        v.pos.resize(cap); v.qual.resize(cap); v.gt.resize(cap); v.ins_qual.resize(cap); v.depth.resize(cap); v.counts.resize(cap * 7);
        check(ctx, call(cap, v.pos.data(), v.gt.data(), v.qual.data(), v.ins_qual.data(), v.depth.data(), v.counts.data(), &v.n_tested, &v.n_calls));
        if (v.n_calls <= cap) break;
        cap = v.n_calls;
    }
}

// `call(cap, rows, &n_rows)` is one of the two library calls with everything before cap bound: asked again when the first answer
// holds more rows than it had room for.  The store must hold exactly the reads whose numbers were noted.
template <typename F>
void tags_fetch(vga_ctx *ctx, PhaseTags &t, uint64_t n_stored, F call)
{
    if (t.read_ids.size() != n_stored)
        throw Error("--haplotag: the phase store holds " + std::to_string(n_stored) + " reads, and " + std::to_string(t.read_ids.size()) + " reads were noted as kept");
    uint64_t cap = std::max<uint64_t>(4096, 4 * n_stored);
    for (;;) {
        t.rows.resize(cap * PH_TAG_COLS);
        check(ctx, call(cap, t.rows.data(), &t.n_rows));
        if (t.n_rows <= cap) break;
        cap = t.n_rows;
    }
    t.rows.resize(t.n_rows * PH_TAG_COLS);
}

// `call(cap, rows, &n_rows)` is one of the two library calls with everything before cap bound: it counts nothing when there are
// more jobs than it had room for, and is asked again
template <typename F>
void hap_counts_fetch(vga_ctx *ctx, HaplotypeCounts &h, uint64_t n_calls, F call)
{
    uint64_t cap = std::max<uint64_t>(4096, 2 * n_calls);
    for (;;) {
        h.rows.resize(cap * HC_ROW);
        check(ctx, call(cap, h.rows.data(), &h.n_rows));
        if (h.n_rows <= cap) break;
        cap = h.n_rows;
    }
    h.rows.resize(h.n_rows * HC_ROW);
}

// `call(cap_rows, table, &n_sets)` is one of the two library calls with everything before cap_rows bound, asked with room for the
// table of the chain's sets (more than PJ_MAX_SETS: refused with the count).  Then the join rule on the table, and per site the
// joined ps and flip.
template <typename F>
void join_fetch(vga_ctx *ctx, PhaseJoin &j, const PhaseLinks &p, uint32_t min_reads, F call)
{
    const size_t n = p.pos.size();
    j.set_ps.clear();
    for (size_t h = 0; h < n; h++)
        if (p.ps[h] == h + 1u) j.set_ps.push_back((uint32_t)(h + 1u));
    const uint64_t S = j.n_sets = j.set_ps.size(), rows = vga_pair_count(S);
    j.table.assign(rows * PJ_COLS + PJ_COLS, 0);  // (an empty store leaves it so)
    uint64_t counted = 0;
    check(ctx, call(rows, j.table.data(), &counted));
    if (counted != S && counted != 0) throw Error("--phase-join: the chain has " + std::to_string(S) + " sets, and " + std::to_string(counted) + " were counted");
    j.set_root.assign(S + 1, 0); j.set_flip.assign(S + 1, 0); j.joins.assign((S + 1) * PJ_JOIN_COLS, 0);
    pj_join(S, j.table.data(), min_reads, j.set_root.data(), j.set_flip.data(), j.joins.data(), &j.n_joins, &j.n_agree, &j.n_conflict);
    j.ps.assign(n + 1, 0); j.flip.assign(n + 1, 0);
    pj_sites(n, p.ps.data(), p.flip.data(), j.set_root.data(), j.set_flip.data(), j.ps.data(), j.flip.data());
}

// `call(cap_groups, reads, table, &n_sets)` is one of the two library calls with everything before cap_groups bound, asked with room
// for the groups of the sets of ps (more than HP_MAX_SETS, or a table of more than HP_MAX_ENTRIES: refused with the counts)
template <typename F>
void hap_paths_fetch(vga_ctx *ctx, HapPaths &h, const std::vector<uint32_t> &ps, size_t n_sites, size_t n_paths, F call)
{
    uint64_t S = 0;
    for (size_t s = 0; s < n_sites; s++) S += ps[s] == s + 1u ? 1u : 0u;
    h.reads.assign(2 * S + 2, 0);  // (an empty store leaves them so)
    h.table.assign(std::min<uint64_t>(2 * S * n_paths, HP_MAX_ENTRIES) * HP_COLS + HP_COLS, 0);
    uint64_t summed = 0;
    check(ctx, call(2 * S, h.reads.data(), h.table.data(), &summed));
    if (summed != S && summed != 0) throw Error("--haplotype-paths: there are " + std::to_string(S) + " sets, and " + std::to_string(summed) + " were summed");
    h.n_sets = S;
}

// ---- the writers.  Each gets its table padded to the sizes it indexes.

void coverage_write(const Index &ix, const Counters &s, const std::string &out_prefix)
{
    const std::vector<uint64_t> &base = s.v[0], &node = s.v[1], &edge = s.v[2];
    std::string nodes = "node\tlength\treads\tbases\n", bases = "node\toffset\tdepth\n", edges = "from\tto\treads\n";
    for (uint64_t id = 1; id <= ix.n_nodes; id++) {
        const uint64_t p0 = ix.node_ref[id - 1].seq_idx, p1 = ix.node_ref[id].seq_idx;
        uint64_t sum = 0;
        for (uint64_t p = p0; p < p1; p++) {
            sum += base[p];
            put_u64(bases, id); bases += '\t'; put_u64(bases, p - p0); bases += '\t'; put_u64(bases, base[p]); bases += '\n';
        }
        put_u64(nodes, id); nodes += '\t'; put_u64(nodes, p1 - p0); nodes += '\t'; put_u64(nodes, node[id - 1]); nodes += '\t';
        put_u64(nodes, sum); nodes += '\n';
        for (uint64_t e = ix.node_ref[id - 1].edge_idx + ix.node_ref[id - 1].edges_to_node; e < ix.node_ref[id].edge_idx; e++) {
            put_u64(edges, id); edges += '\t'; put_u64(edges, id_of(ix.edges[e])); edges += '\t'; put_u64(edges, edge[e]); edges += '\n';
        }
    }
    write_file(out_prefix + "-coverage-nodes.tsv", nodes);
    write_file(out_prefix + "-coverage-bases.tsv", bases);
    write_file(out_prefix + "-coverage-edges.tsv", edges);
}

void pileup_write(const Index &ix, const Counters &s, const std::string &out_prefix)
{
    std::string t = "node\toffset\tref\tA\tC\tG\tT\tN\tdel\tins\n";
    for (uint64_t id = 1; id <= ix.n_nodes; id++) {
        const uint64_t p0 = ix.node_ref[id - 1].seq_idx, p1 = ix.node_ref[id].seq_idx;
        for (uint64_t p = p0; p < p1; p++) {
            put_u64(t, id); t += '\t'; put_u64(t, p - p0); t += '\t'; t += ix.seq_fwd[p];
            for (int c = 0; c < 7; c++) { t += '\t'; put_u64(t, s.v[0][p * 7 + (uint64_t)c]); }
            t += '\n';
        }
    }
    write_file(out_prefix + "-pileup.tsv", t);
}

void variant_write(const Index &ix, const VariantCalls &v, const std::string &out_prefix)
{
    static const char ALLELES[] = "ACGT-";
    static const char *const STATES[] = {".", "het", "hom"};
    std::string t = "node\toffset\tref\tgt\tqual\tins\tins_qual\tdepth\tA\tC\tG\tT\tN\tdel\tins_count\n";
    uint64_t id = 1;  // the calls come in base order: the node moves forward only
    for (uint64_t j = 0; j < v.n_calls; j++) {
        const uint64_t p = v.pos[j];
        while (id < ix.n_nodes && ix.node_ref[id].seq_idx <= p) id++;
        const uint32_t g = v.gt[j];
        put_u64(t, id); t += '\t'; put_u64(t, p - ix.node_ref[id - 1].seq_idx); t += '\t'; t += ix.seq_fwd[p]; t += '\t';
        t += ALLELES[g & 7u]; t += '/'; t += ALLELES[(g >> 3) & 7u]; t += '\t'; put_u64(t, v.qual[j]); t += '\t';
        t += STATES[(g >> 6) < 3u ? (g >> 6) : 0u]; t += '\t'; put_u64(t, v.ins_qual[j]); t += '\t'; put_u64(t, v.depth[j]);
        for (int c = 0; c < 7; c++) { t += '\t'; put_u64(t, v.counts[j * 7 + (uint64_t)c]); }
        t += '\n';
    }
    write_file(out_prefix + "-variants.tsv", t);
}

// `call(cap, first, len, last, state, qual, depth, reads, &n_distinct, &n_calls)` is one of the two library calls with everything
// before cap bound: asked again when the first answer holds more calls than it had room for
template <typename F>
void deletion_fetch(vga_ctx *ctx, DeletionCalls &d, F call)
{
    uint64_t cap = 4096;
    for (;;) {
        d.first.resize(cap); d.len.resize(cap); d.last.resize(cap); d.qual.resize(cap); d.state.resize(cap); d.depth.resize(cap); d.reads.resize(cap);
        check(ctx, call(cap, d.first.data(), d.len.data(), d.last.data(), d.state.data(), d.qual.data(), d.depth.data(), d.reads.data(), &d.n_distinct, &d.n_calls));
        if (d.n_calls <= cap) break;
        cap = d.n_calls;
    }
}

// <out>-deletions.tsv: one line per reported group, in sort order
void deletion_write(const Index &ix, const DeletionCalls &d, MapOutput &out, const std::string &out_prefix)
{
    out.n_deletion_runs = d.n_events + d.n_end_runs; out.n_deletion_alignments = d.n_alignments; out.n_deletion_end_runs = d.n_end_runs;
    out.n_deletion_distinct = d.n_distinct; out.n_deletion_calls = d.n_calls;
    if (out_prefix.empty()) return;
    std::string t = "node\toffset\tend_node\tend_offset\tlength\tstate\tqual\tdepth\treads\n";
    auto node_of = [&](uint64_t pos) {  // the 1-based id of the node that holds the base: the last whose start is not behind it
        uint64_t lo = 1, hi = ix.n_nodes + 1;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) / 2;
            if (ix.node_ref[mid - 1].seq_idx <= pos) lo = mid; else hi = mid;
        }
        return lo;
    };
    for (uint64_t i = 0; i < d.n_calls; i++) {
        const uint64_t a = node_of(d.first[i]), b = node_of(d.last[i]);
        put_u64(t, a); t += '\t'; put_u64(t, d.first[i] - ix.node_ref[a - 1].seq_idx); t += '\t';
        put_u64(t, b); t += '\t'; put_u64(t, d.last[i] - ix.node_ref[b - 1].seq_idx); t += '\t';
        put_u64(t, d.len[i]); t += '\t'; t += dl_state_name(d.state[i]); t += '\t'; put_u64(t, d.qual[i]); t += '\t';
        put_u64(t, d.depth[i]); t += '\t'; put_u64(t, d.reads[i]); t += '\n';
    }
    write_file(out_prefix + "-deletions.tsv", t);
}

// one line per called site: where it is and what the variant call says of it, then length (1 .. 8, or >8), the reads of that
// length, the letters and the reads of each
void insertion_write(const Index &ix, const VariantCalls &v, const InsertionCalls &c, MapOutput &out, const std::string &out_prefix)
{
    static const char *const STATES[] = {".", "het", "hom"};
    std::string t = "node\toffset\tstate\tins_qual\tdepth\tins_count\tlength\tlength_reads\tseq\tseq_reads\n";
    uint64_t id = 1;  // the sites come in base order: the node moves forward only
    out.n_insertion_sites = c.site.size();
    out.n_insertion_long = 0;
    for (size_t s = 0; s < c.site.size(); s++) {
        const uint64_t j = c.site[s], p = v.pos[j];
        while (id < ix.n_nodes && ix.node_ref[id].seq_idx <= p) id++;
        const uint32_t len = c.length[s], kept = std::min<uint32_t>(len, IA_MAX_LEN);
        out.n_insertion_long += len > IA_MAX_LEN ? 1u : 0u;
        put_u64(t, id); t += '\t'; put_u64(t, p - ix.node_ref[id - 1].seq_idx); t += '\t'; t += STATES[(v.gt[j] >> 6) < 3u ? (v.gt[j] >> 6) : 0u]; t += '\t';
        put_u64(t, v.ins_qual[j]); t += '\t'; put_u64(t, v.depth[j]); t += '\t'; put_u64(t, v.counts[j * 7 + 6]); t += '\t';
        if (len > IA_MAX_LEN) t += ">8"; else put_u64(t, len);
        t += '\t'; put_u64(t, c.length_reads[s]); t += '\t';
        for (uint32_t k = 0; k < kept; k++) t += (char)c.seq[s * IA_MAX_LEN + k];
        if (!kept) t += '.';
        t += '\t';
        for (uint32_t k = 0; k < kept; k++) { if (k) t += ','; put_u64(t, c.seq_reads[s * IA_MAX_LEN + k]); }
        if (!kept) t += '.';
        t += '\n';
    }
    if (!out_prefix.empty()) write_file(out_prefix + "-insertions.tsv", t);
}

// one line per heterozygous site: where it is, the genotype with haplotype a first, the set, the link that joined it (how many
// sites back, 0 for none) with the reads for and against it, and what the reads show at the site
// (the lines under the sets ps and flip: the chain's own, or the joined ones of --phase-join; the link columns are the chain's)
std::string phase_text(const Index &ix, const PhaseLinks &p, const std::vector<uint32_t> &ps, const std::vector<uint8_t> &flip)
{
    static const char ALLELES[] = "ACGT-";
    const size_t n = p.pos.size();
    const std::vector<uint8_t> &link_d = p.link_d;
    std::string t = "node\toffset\tgt\tps\tlink\tcis\ttrans\tx_reads\ty_reads\tother_reads\n";
    uint64_t id = 1;  // the sites come in base order: the node moves forward only
    for (size_t h = 0; h < n; h++) {
        const uint64_t at = p.pos[h];
        while (id < ix.n_nodes && ix.node_ref[id].seq_idx <= at) id++;
        uint64_t cis = 0, trans = 0;
        if (link_d[h]) {
            const uint32_t *l = p.links.data() + ((h - link_d[h]) * PH_WINDOW + (link_d[h] - 1u)) * PH_LINK_COLS;
            cis = (uint64_t)l[0] + l[3]; trans = (uint64_t)l[1] + l[2];
        }
        put_u64(t, id); t += '\t'; put_u64(t, at - ix.node_ref[id - 1].seq_idx); t += '\t';
        t += ALLELES[flip[h] ? p.y[h] : p.x[h]]; t += '|'; t += ALLELES[flip[h] ? p.x[h] : p.y[h]]; t += '\t';
        put_u64(t, ps[h]); t += '\t'; put_u64(t, link_d[h]); t += '\t'; put_u64(t, cis); t += '\t'; put_u64(t, trans);
        for (uint32_t c = 0; c < PH_SITE_COLS; c++) { t += '\t'; put_u64(t, p.site_reads[h * PH_SITE_COLS + c]); }
        t += '\n';
    }
    return t;
}

void phase_write(const Index &ix, PhaseLinks &p, uint32_t min_links, MapOutput &out, const std::string &out_prefix)
{
    p.chain(min_links);
    out.n_phase_sites = p.pos.size(); out.n_phase_sets = 0; out.n_phase_reads = p.n_reads;
    for (size_t h = 0; h < p.pos.size(); h++) out.n_phase_sets += p.link_d[h] == 0 ? 1u : 0u;
    const std::string t = phase_text(ix, p, p.ps, p.flip);
    if (!out_prefix.empty()) write_file(out_prefix + "-phase.tsv", t);
}

// <out>-phase-joined.tsv: the lines of <out>-phase.tsv under the joined sets; <out>-phase-sets.tsv: one line per chain set, its
// sites, the reads tagged a and b in it (the diagonal of the table), the set that names its component and its parity against it;
// <out>-phase-joins.tsv: one line per accepted link, in the order of the join
void phase_join_write(const Index &ix, const PhaseLinks &p, const PhaseJoin &j, MapOutput &out, const std::string &out_prefix)
{
    const uint64_t S = j.n_sets;
    out.n_join_sets = S; out.n_joins = j.n_joins; out.n_join_agree = j.n_agree; out.n_join_conflict = j.n_conflict;
    if (out_prefix.empty()) return;
    write_file(out_prefix + "-phase-joined.tsv", phase_text(ix, p, j.ps, j.flip));
    std::vector<uint64_t> sites(S + 1, 0);
    for (size_t h = 0; h < p.pos.size(); h++) sites[(size_t)(std::lower_bound(j.set_ps.begin(), j.set_ps.end(), p.ps[h]) - j.set_ps.begin())]++;
    std::string t = "ps\tsites\treads_a\treads_b\tjoined_ps\tflip\n";
    for (uint64_t s = 0; s < S; s++) {
        const uint32_t *n = j.table.data() + vga_pair_index(S, s, s) * PJ_COLS;
        put_u64(t, j.set_ps[s]); t += '\t'; put_u64(t, sites[s]); t += '\t'; put_u64(t, n[0]); t += '\t'; put_u64(t, n[3]); t += '\t';
        put_u64(t, j.set_ps[j.set_root[s]]); t += '\t'; put_u64(t, j.set_flip[s]); t += '\n';
    }
    write_file(out_prefix + "-phase-sets.tsv", t);
    t = "ps_a\tps_b\tcis\ttrans\trel\n";
    for (uint64_t k = 0; k < j.n_joins; k++) {
        const uint32_t *l = j.joins.data() + k * PJ_JOIN_COLS;
        put_u64(t, j.set_ps[l[0]]); t += '\t'; put_u64(t, j.set_ps[l[1]]); t += '\t'; put_u64(t, l[2]); t += '\t'; put_u64(t, l[3]); t += '\t';
        t += l[3] > l[2] ? "trans" : "cis"; t += '\n';
    }
    write_file(out_prefix + "-phase-joins.tsv", t);
}

// One block per ranked group (reads above 0) in (ps, a before b) order: the best `top` paths (0: all) by the rank rule of
// vga_hap_paths.hpp (hp_rank), each with its cost, its cost above rank 1, the reads it fits best and the paths tied at the minimum.
// The call of the set with the most scored tagged reads (the smallest ps on a tie) goes to `out`.
void haplotype_paths_write(const MapOptions &opt, const std::vector<uint32_t> &ps, size_t n_sites, const HapPaths &h, uint64_t n_kept, MapOutput &out,
                           const std::string &out_prefix)
{
    const size_t np = opt.paths.n_paths();
    const uint64_t S = h.n_sets;
    std::vector<uint32_t> set_ps, order(np + 1);
    for (size_t s = 0; s < n_sites; s++)
        if (ps[s] == s + 1u) set_ps.push_back((uint32_t)(s + 1u));
    std::string t = "ps\thap\treads\trank\tpath\tcost\tmargin\tbest\ttied\n";
    out.n_hap_path_sets = S; out.n_hap_path_groups = 0; out.n_hap_path_scored = h.n_scored; out.n_hap_path_kept = n_kept;
    uint64_t largest = 0, largest_reads = 0;
    for (uint64_t s = 0; s < S; s++)
        if (h.reads[2 * s] + h.reads[2 * s + 1] > largest_reads) { largest = s; largest_reads = h.reads[2 * s] + h.reads[2 * s + 1]; }
    std::string name[2] = {".", "."};
    uint64_t margin[2] = {0, 0}, tied_of[2] = {0, 0};
    for (uint64_t g = 0; g < 2 * S; g++) {
        if (h.reads[g] == 0) continue;
        out.n_hap_path_groups++;
        const uint64_t *e = h.table.data() + g * np * HP_COLS;
        const uint32_t tied = hp_rank((uint32_t)np, e, order.data());
        const size_t rows = opt.haplotype_paths_top ? std::min<size_t>(opt.haplotype_paths_top, np) : np;
        for (size_t k = 0; k < rows; k++) {
            const uint64_t *c = e + (uint64_t)order[k] * HP_COLS;
            put_u64(t, set_ps[g / 2]); t += '\t'; t += g & 1u ? 'b' : 'a'; t += '\t'; put_u64(t, h.reads[g]); t += '\t'; put_u64(t, k + 1); t += '\t';
            t += opt.paths.names[order[k]]; t += '\t'; put_u64(t, c[0]); t += '\t'; put_u64(t, c[0] - e[(uint64_t)order[0] * HP_COLS]); t += '\t'; put_u64(t, c[1]);
            t += '\t'; put_u64(t, tied); t += '\n';
        }
        if (g / 2 == largest) {
            name[g & 1u] = opt.paths.names[order[0]];
            margin[g & 1u] = np > 1 ? e[(uint64_t)order[1] * HP_COLS] - e[(uint64_t)order[0] * HP_COLS] : 0;
            tied_of[g & 1u] = tied;
        }
    }
    if (out.n_hap_path_groups) {
        std::string &c = out.hap_path_call;
        c = "ps "; put_u64(c, set_ps[largest]); c += ": " + name[0] + " | " + name[1] + " (reads "; put_u64(c, h.reads[2 * largest]); c += " | ";
        put_u64(c, h.reads[2 * largest + 1]); c += ", margins "; put_u64(c, margin[0]); c += " | "; put_u64(c, margin[1]); c += ", tied "; put_u64(c, tied_of[0]);
        c += " | "; put_u64(c, tied_of[1]); c += ")";
    }
    if (!out_prefix.empty()) write_file(out_prefix + "-haplotype-paths.tsv", t);
}

// One line per path of at least abundance_min parts per million, by theta descending, then in P-line order; the header alone
// without a call.
void abundance_write(const MapOptions &opt, const Abundance &a, MapOutput &out, const std::string &out_prefix)
{
    const size_t np = opt.paths.n_paths();
    out.n_abundance_scored = a.n_scored; out.n_abundance_kept = a.n_kept; out.abundance_iterations = a.iterations; out.abundance_converged = a.converged != 0;
    out.abundance_ppm.clear();
    std::string t = "rank\tpath\tppm\ttheta\treads_q16\tbest\n";
    if (a.n_scored) {
        std::vector<uint32_t> order(np);
        for (uint32_t p = 0; p < np; p++) order[p] = p;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return a.theta[x] > a.theta[y]; });
        for (uint32_t p : order) {
            const uint64_t ppm = vga_ab_ppm(a.theta[p]);
            if (ppm < opt.abundance_min) continue;
            out.abundance_ppm.push_back(ppm);
            put_u64(t, out.abundance_ppm.size()); t += '\t'; t += opt.paths.names[p]; t += '\t'; put_u64(t, ppm); t += '\t'; put_u64(t, a.theta[p]); t += '\t';
            put_u64(t, a.reads_q16[p]); t += '\t'; put_u64(t, a.best[p]); t += '\n';
        }
    }
    if (!out_prefix.empty()) write_file(out_prefix + "-path-abundance.tsv", t);
}

// one line per (kept read, phase set) in which a site votes: the read as the input file numbers it, the set as <out>-phase.tsv
// numbers it, the haplotype with more votes (. on a tie) and the votes; by read, then by set.  The rows come in store order, which
// is read order unless several contexts kept the reads.
void haplotag_write(const PhaseTags &t, MapOutput &out, const std::string &out_prefix)
{
    std::vector<uint64_t> at(t.n_rows);
    for (uint64_t i = 0; i < t.n_rows; i++) at[i] = i;
    auto read_of = [&](uint64_t i) { return t.read_ids[t.rows[i * PH_TAG_COLS]]; };
    auto before = [&](uint64_t a, uint64_t b) { return read_of(a) < read_of(b); };
    if (!std::is_sorted(at.begin(), at.end(), before)) std::stable_sort(at.begin(), at.end(), before);
    std::string s = "read\tps\thap\tvotes_a\tvotes_b\n";
    out.n_haplotag_rows = t.n_rows; out.n_haplotag_a = out.n_haplotag_b = out.n_haplotag_tied = 0;
    for (uint64_t i : at) {
        const uint32_t *r = t.rows.data() + i * PH_TAG_COLS;
        const char hap = r[2] > r[3] ? 'a' : r[3] > r[2] ? 'b' : '.';
        (hap == 'a' ? out.n_haplotag_a : hap == 'b' ? out.n_haplotag_b : out.n_haplotag_tied)++;
        put_u64(s, read_of(i)); s += '\t'; put_u64(s, r[1]); s += '\t'; s += hap; s += '\t'; put_u64(s, r[2]); s += '\t'; put_u64(s, r[3]); s += '\n';
    }
    if (!out_prefix.empty()) write_file(out_prefix + "-haplotag.tsv", s);
}

// one line per job (a row of <out>-variants.tsv, a phase set whose sites span it) at which a tagged read of the set shows anything:
// where it is, the set, the haploid call of each haplotype (hc_call), the reads each call rests on and the seven counts of each
void haplotype_calls_write(const Index &ix, const VariantCalls &v, const HaplotypeCounts &h, MapOutput &out, const std::string &out_prefix)
{
    std::string t = "node\toffset\tref\tps\ta\tb\ta_obs\tb_obs\ta_A\ta_C\ta_G\ta_T\ta_N\ta_del\ta_ins\tb_A\tb_C\tb_G\tb_T\tb_N\tb_del\tb_ins\n";
    uint64_t id = 1;  // the jobs come in base order: the node moves forward only
    out.n_hapcall_jobs = h.n_rows; out.n_hapcall_rows = out.n_hapcall_differ = 0;
    for (uint64_t j = 0; j < h.n_rows; j++) {
        const uint32_t *r = h.rows.data() + j * HC_ROW, *a = r + 2, *b = a + HC_COLS;
        uint64_t obs[2] = {0, 0};
        for (uint32_t k = 0; k < HC_COL_INS; k++) { obs[0] += a[k]; obs[1] += b[k]; }
        if (obs[0] + obs[1] + a[HC_COL_INS] + b[HC_COL_INS] == 0) continue;
        const uint64_t p = v.pos[r[0]];
        while (id < ix.n_nodes && ix.node_ref[id].seq_idx <= p) id++;
        const uint32_t ca = hc_call(a), cb = hc_call(b);
        char text[3];
        out.n_hapcall_rows++;
        out.n_hapcall_differ += (ca & 7u) < HC_CALL_NONE && (cb & 7u) < HC_CALL_NONE && ca != cb ? 1u : 0u;
        put_u64(t, id); t += '\t'; put_u64(t, p - ix.node_ref[id - 1].seq_idx); t += '\t'; t += ix.seq_fwd[p]; t += '\t'; put_u64(t, r[1]); t += '\t';
        hc_call_text(ca, text); t += text; t += '\t'; hc_call_text(cb, text); t += text; t += '\t'; put_u64(t, obs[0]); t += '\t'; put_u64(t, obs[1]);
        for (uint32_t k = 0; k < 2u * HC_COLS; k++) { t += '\t'; put_u64(t, a[k]); }
        t += '\n';
    }
    if (!out_prefix.empty()) write_file(out_prefix + "-haplotype-calls.tsv", t);
}

void path_support_write(const MapOptions &opt, const Counters &s, const std::string &rows, const std::string &out_prefix)
{
    const size_t np = opt.paths.n_paths();
    std::string paths = "path\tsteps\tlength\tsum_bases\tsum_edges\ttop\ttop_alone\n";
    for (size_t p = 0; p < np; p++) {
        paths += opt.paths.names[p]; paths += '\t'; put_u64(paths, opt.paths.step_off[p + 1] - opt.paths.step_off[p]); paths += '\t';
        put_u64(paths, opt.paths.length[p]);
        for (const auto &x : s.v) { paths += '\t'; put_u64(paths, x[p]); }
        paths += '\n';
    }
    write_file(out_prefix + "-path-support.tsv", paths);
    write_file(out_prefix + "-path-support-reads.tsv", "read\tpath\tbases\tedges\n" + rows);
}

// (length: |seq_p|, the bases of all the steps of the path, whichever way they are visited)
void path_edit_write(const Index &ix, const MapOptions &opt, const Counters &s, const std::string &rows, const std::string &out_prefix)
{
    const size_t np = opt.paths.n_paths();
    std::string paths = "path\tsteps\tlength\tscored\tsum_edit\tbest\tbest_alone\n";
    for (size_t p = 0; p < np; p++) {
        paths += opt.paths.names[p]; paths += '\t'; put_u64(paths, opt.paths.step_off[p + 1] - opt.paths.step_off[p]); paths += '\t';
        uint64_t len = 0;
        for (uint64_t t = opt.paths.step_off[p]; t < opt.paths.step_off[p + 1]; t++) {
            const uint64_t id = id_of(opt.paths.steps[t]);
            len += ix.node_ref[id].seq_idx - ix.node_ref[id - 1].seq_idx;
        }
        put_u64(paths, len);
        for (const auto &x : s.v) { paths += '\t'; put_u64(paths, x[p]); }
        paths += '\n';
    }
    write_file(out_prefix + "-path-edit.tsv", paths);
    write_file(out_prefix + "-path-edit-reads.tsv", "read\tpath\tedit\n" + rows);
}

// The pairs whose sums are not (0, 0), from the best down: by sum_bases, then sum_edges, both descending, then the homozygous
// pair before a heterozygous one, then p, then q.
void genotype_write(const MapOptions &opt, const Counters &s, MapOutput &out, const std::string &out_prefix)
{
    const size_t np = opt.paths.n_paths();
    struct Pair { uint32_t p, q; uint64_t at; };
    std::vector<Pair> ranked;
    for (uint32_t p = 0; p < np; p++)
        for (uint32_t q = p; q < np; q++) {
            const uint64_t at = vga_pair_index(np, p, q);
            if (s.v[0][at] || s.v[1][at]) ranked.push_back({p, q, at});
        }
    std::sort(ranked.begin(), ranked.end(), [&](const Pair &a, const Pair &b) {
        if (s.v[0][a.at] != s.v[0][b.at]) return s.v[0][a.at] > s.v[0][b.at];
        if (s.v[1][a.at] != s.v[1][b.at]) return s.v[1][a.at] > s.v[1][b.at];
        if ((a.p == a.q) != (b.p == b.q)) return a.p == a.q;
        return a.p != b.p ? a.p < b.p : a.q < b.q;
    });
    out.n_genotype_pairs = ranked.size();
    if (!ranked.empty()) {
        out.genotype_a = opt.paths.names[ranked[0].p]; out.genotype_b = opt.paths.names[ranked[0].q];
        out.genotype_sum_bases = s.v[0][ranked[0].at]; out.genotype_sum_edges = s.v[1][ranked[0].at];
    }
    if (out_prefix.empty()) return;
    std::string t = "rank\tpath_a\tpath_b\tsum_bases\tsum_edges\tprefer_a\tprefer_b\n";
    const size_t rows = opt.genotype_top ? std::min<size_t>(opt.genotype_top, ranked.size()) : ranked.size();
    for (size_t i = 0; i < rows; i++) {
        put_u64(t, i + 1); t += '\t'; t += opt.paths.names[ranked[i].p]; t += '\t'; t += opt.paths.names[ranked[i].q];
        for (const auto &x : s.v) { t += '\t'; put_u64(t, x[ranked[i].at]); }
        t += '\n';
    }
    write_file(out_prefix + "-genotype.tsv", t);
}

// Every pair from the cheapest up: by cost, then the homozygous pair before a heterozygous one, then p, then q.  No row scored:
// no call, and a table with its header only.
void likelihood_write(const MapOptions &opt, const Counters &s, MapOutput &out, const std::string &out_prefix)
{
    const size_t np = opt.paths.n_paths();
    const uint64_t n_scored = s.n[0];
    struct Pair { uint32_t p, q; uint64_t cost; };
    std::vector<Pair> ranked;
    if (n_scored)
        for (uint32_t p = 0; p < np; p++)
            for (uint32_t q = p; q < np; q++) ranked.push_back({p, q, s.v[0][vga_pair_index(np, p, q)]});
    std::sort(ranked.begin(), ranked.end(), [](const Pair &a, const Pair &b) {
        if (a.cost != b.cost) return a.cost < b.cost;
        if ((a.p == a.q) != (b.p == b.q)) return a.p == a.q;
        return a.p != b.p ? a.p < b.p : a.q < b.q;
    });
    out.n_likelihood_scored = n_scored;
    if (!ranked.empty()) {
        out.likelihood_a = opt.paths.names[ranked[0].p]; out.likelihood_b = opt.paths.names[ranked[0].q];
        out.likelihood_cost = ranked[0].cost;
        out.likelihood_next = ranked.size() > 1 ? ranked[1].cost - ranked[0].cost : 0;
    }
    if (out_prefix.empty()) return;
    std::string t = "rank\tpath_a\tpath_b\tcost\tmargin\n";
    const size_t rows = opt.genotype_top ? std::min<size_t>(opt.genotype_top, ranked.size()) : ranked.size();
    for (size_t i = 0; i < rows; i++) {
        put_u64(t, i + 1); t += '\t'; t += opt.paths.names[ranked[i].p]; t += '\t'; t += opt.paths.names[ranked[i].q]; t += '\t';
        put_u64(t, ranked[i].cost); t += '\t'; put_u64(t, ranked[i].cost - ranked[0].cost); t += '\n';
    }
    write_file(out_prefix + "-genotype-likelihood.tsv", t);
}

}  // namespace

void check_aligner(const MapOptions &opt)
{
    if (opt.genotype_likelihood && !opt.also_align) throw Error("--genotype-likelihood calls from alignments: it needs --also-align");
    if (opt.genotype_likelihood && opt.paths.n_paths() == 0) throw Error("--genotype-likelihood: the graph has no P line");
    if (opt.genotype_likelihood && !likelihood_params_ok(opt)) throw Error("--genotype-likelihood: --genotype-lambda is 1 to 4096 and --genotype-cap 1 to 255");
    if (opt.genotype_from_edit && !opt.genotype_likelihood) throw Error("--genotype-from has no meaning without --genotype-likelihood");
    if (opt.path_edit && !opt.also_align) throw Error("--path-edit scores alignments: it needs --also-align");
    if (opt.path_edit && opt.paths.n_paths() == 0) throw Error("--path-edit: the graph has no P line");
    if (opt.genotype && !opt.also_align) throw Error("--genotype calls from alignments: it needs --also-align");
    if (opt.genotype && opt.paths.n_paths() == 0) throw Error("--genotype: the graph has no P line");
    if (opt.path_support && !opt.also_align) throw Error("--path-support scores alignments: it needs --also-align");
    if (opt.path_support && opt.paths.n_paths() == 0) throw Error("--path-support: the graph has no P line");
    if (opt.pileup && !opt.also_align) throw Error("--pileup counts alignments: it needs --also-align");
    if (opt.call_variants && !opt.also_align) throw Error("--call-variants calls from alignments: it needs --also-align");
    if (opt.call_variants && !variant_params_ok(opt)) throw Error("--call-variants: --call-error is 257 to 8192 and --call-min-depth at least 1");
    if (opt.call_insertions && !opt.call_variants) throw Error("--call-insertions calls at the sites of --call-variants: it needs --call-variants");
    if (opt.call_deletions && !opt.also_align) throw Error("--call-deletions calls from alignments: it needs --also-align");
    if (opt.call_deletions && !opt.call_variants) throw Error("--call-deletions calls with the depth and the parameters of --call-variants: it needs --call-variants");
    if (opt.phase && !opt.call_variants) throw Error("--phase links the heterozygous sites of --call-variants: it needs --call-variants");
    if (opt.phase && (opt.phase_min_links < 1 || opt.phase_min_links > PH_MIN_LINKS_MAX)) throw Error("--phase-min-links is 1 to 65535");
    if (opt.haplotag && !opt.phase) throw Error("--haplotag assigns reads to the haplotypes of the phase sets of --phase: it needs --phase");
    if (opt.haplotype_calls && !opt.haplotag) throw Error("--haplotype-calls counts what the reads tagged by --haplotag show: it needs --haplotag");
    if (opt.phase_join && !opt.phase) throw Error("--phase-join joins the phase sets of --phase: it needs --phase");
    if (opt.phase_join && (opt.phase_join_min_reads < 1 || opt.phase_join_min_reads > PJ_MIN_READS_MAX)) throw Error("--phase-join-min-reads is 1 to 65535");
    if (opt.haplotype_paths && !opt.phase) throw Error("--haplotype-paths types the haplotypes of the phase sets of --phase: it needs --phase");
    if (opt.haplotype_paths && opt.paths.n_paths() == 0) throw Error("--haplotype-paths: the graph has no P line");
    if (opt.haplotype_paths && (opt.haplotype_paths_cap < 1 || opt.haplotype_paths_cap > HP_CAP_MAX)) throw Error("--haplotype-paths-cap is 1 to 255");
    if (opt.haplotype_paths_from_edit && !opt.haplotype_paths) throw Error("--haplotype-paths-from has no meaning without --haplotype-paths");
    if (opt.path_abundance && !opt.also_align) throw Error("--path-abundance estimates from alignments: it needs --also-align");
    if (opt.path_abundance && opt.paths.n_paths() == 0) throw Error("--path-abundance: the graph has no P line");
    if (opt.path_abundance && (opt.abundance_cap < 1 || opt.abundance_cap > AB_CAP_MAX || !vga_ab_params_ok(opt.abundance_lambda, opt.abundance_iters, opt.abundance_tol)))
        throw Error("--path-abundance: --abundance-lambda is 1 to 4096, --abundance-cap 1 to 255, --abundance-iters 1 to 100000 and --abundance-tol 0 to 16777216");
    if (opt.abundance_from_edit && !opt.path_abundance) throw Error("--abundance-from has no meaning without --path-abundance");
    if ((opt.coverage || opt.coverage_only) && !opt.also_align) throw Error("--coverage counts alignments: it needs --also-align");
    if (opt.poa_aligner != "abpoa") {
        if (opt.poa_aligner == "rspoa") throw Error("the rspoa aligner is not available in the MI355X build yet; use -p abpoa");
        throw Error("POA Aligner not recognized");  // map_main.rs:67
    }
}

Tables::Tables(const Index &ix, const MapOptions &opt) : ix_(ix), opt_(opt) {}

void Tables::begin(vga_ctx *ctx) const
{
    if (coverage()) check(ctx, vga_coverage_begin(ctx));
    if (scoring()) {  // path support and what is built on it
        check(ctx, vga_path_support_begin(ctx, (uint32_t)opt_.paths.n_paths(), opt_.paths.step_off.data(), opt_.paths.steps.data(), nullptr));
        if (edit()) check(ctx, vga_path_edit_begin(ctx));
        if (opt_.genotype) check(ctx, vga_genotype_begin(ctx));
        if (opt_.genotype_likelihood) check(ctx, vga_genotype_lik_begin(ctx, opt_.genotype_lambda, opt_.genotype_cap));
        if (opt_.genotype_likelihood && opt_.genotype_from_edit) check(ctx, vga_genotype_lik_source(ctx, VGA_GL_FROM_EDIT));
        if (abundance()) check(ctx, vga_path_abundance_begin(ctx, opt_.abundance_cap, opt_.abundance_from_edit ? VGA_AB_FROM_EDIT : VGA_AB_FROM_SUPPORT));
    }
    if (piling()) check(ctx, vga_pileup_begin(ctx));
    if (inserting()) check(ctx, vga_insertion_begin(ctx));
    if (deleting()) check(ctx, vga_deletion_begin(ctx));
    if (phasing()) check(ctx, vga_phase_begin(ctx));
    if (hap_typing()) check(ctx, vga_haplotype_paths_begin(ctx, opt_.haplotype_paths_cap, opt_.haplotype_paths_from_edit ? VGA_HP_FROM_EDIT : VGA_HP_FROM_SUPPORT));
}

void Tables::chunk_rows(vga_ctx *ctx, uint64_t b0, uint64_t n, const uint8_t *aligned, ReadRows &rows, const std::function<void(const char *)> &mark)
{
    const size_t np = opt_.paths.n_paths();
    if (tagging())  // the store keeps the reported alignments of the call in read order
        for (uint64_t r = 0; r < n; r++)
            if (aligned[r]) tags_.read_ids.push_back(b0 + r);
    // one line per pair (aligned read, path) that keep(at) lets through: the read, the path, then the pair's value in each matrix
    auto put_rows = [&](std::string &dst, std::initializer_list<const std::vector<uint32_t> *> matrices, auto keep) {
        for (uint64_t r = 0; r < n; r++)
            for (size_t p = 0; aligned[r] && p < np; p++)
                if (keep(r * np + p)) {
                    put_u64(dst, b0 + r); dst += '\t'; put_u64(dst, p);
                    for (const std::vector<uint32_t> *m : matrices) { dst += '\t'; put_u64(dst, (*m)[r * np + p]); }
                    dst += '\n';
                }
    };
    if (opt_.path_support) {  // the reads x paths table
        std::vector<uint32_t> pb(n * np + 1), pe(n * np + 1);
        check(ctx, vga_path_support_last(ctx, n, pb.data(), pe.data()));
        put_rows(rows.path, {&pb, &pe}, [&](size_t at) { return pb[at] || pe[at]; });
        mark("path support rows");
    }
    if (opt_.path_edit) {  // the scored pairs of the reads x paths edit distances
        std::vector<uint32_t> ed(n * np + 1);
        check(ctx, vga_path_edit_last(ctx, n, ed.data()));
        put_rows(rows.edit, {&ed}, [&](size_t at) { return ed[at] != 0xFFFFFFFFu; });
        mark("path edit rows");
    }
}

void Tables::take(vga_ctx *ctx, uint32_t slot, bool call_now)
{
    const size_t np = opt_.paths.n_paths(), n_pairs = vga_pair_count(np);
    if (coverage()) {
        Counters t;
        std::vector<uint32_t> b(ix_.seq_length + 1), nd(ix_.n_nodes + 1), ed(ix_.n_edges + 1);
        check(ctx, vga_coverage_read(ctx, b.data(), nd.data(), ed.data(), &t.n[0]));
        t.v = {widen(b, ix_.seq_length), widen(nd, ix_.n_nodes), widen(ed, ix_.n_edges)};
        coverage_.add(t);
    }
    if (scoring()) {
        Counters t;
        t.pad({np, np, np, np});
        check(ctx, vga_path_support_read(ctx, t.v[0].data(), t.v[1].data(), t.v[2].data(), t.v[3].data(), &t.n[0], &t.n[1]));
        paths_.add(t);
    }
    if (opt_.genotype) {
        Counters t;
        t.pad({n_pairs, n_pairs, n_pairs, n_pairs});
        check(ctx, vga_genotype_read(ctx, n_pairs, t.v[0].data(), t.v[1].data(), t.v[2].data(), t.v[3].data()));
        pairs_.add(t);
    }
    if (opt_.genotype_likelihood) {
        Counters t;
        t.pad({n_pairs});
        check(ctx, vga_genotype_lik_read(ctx, n_pairs, t.v[0].data(), &t.n[0]));
        costs_.add(t);
    }
    if (edit()) {
        Counters t;
        t.pad({np, np, np, np});
        check(ctx, vga_path_edit_read(ctx, t.v[0].data(), t.v[1].data(), t.v[2].data(), t.v[3].data(), &t.n[0], &t.n[1]));
        edit_.add(t);
    }
    if (abundance()) {
        Abundance &a = abundance_;
        check(ctx, vga_path_abundance_store(ctx, 0, nullptr, nullptr, &a.n_kept));
        if (call_now) {  // from the context's own store
            a.theta.assign(np + 1, 0); a.reads_q16.assign(np + 1, 0); a.best.assign(np + 1, 0);
            check(ctx, vga_path_abundance(ctx, opt_.abundance_lambda, opt_.abundance_iters, opt_.abundance_tol, a.theta.data(), a.reads_q16.data(), a.best.data(),
                                          &a.n_scored, &a.iterations, &a.converged));
        } else {  // the whole store for the estimate from all of them: n_paths + 1 bytes per reported alignment
            uint64_t n_rows = a.n_kept;
            a.deficits.assign(n_rows * np + 1, 0); a.scored.assign(n_rows + 1, 0);
            check(ctx, vga_path_abundance_store(ctx, n_rows, a.deficits.data(), a.scored.data(), &n_rows));
            if (n_rows != a.n_kept) throw Error("--path-abundance: the store of slot " + std::to_string(slot) + " changed while it was read");
            a.deficits.resize(n_rows * np); a.scored.resize(n_rows);
        }
    }
    // (VGA_TRACE: what each of the two routes to the sites costs at the device's end, tests/prof_variant.py)
    const auto t0 = std::chrono::steady_clock::now();
    if (opt_.pileup || (opt_.call_variants && !call_now)) {
        Counters t;
        std::vector<uint32_t> c(ix_.seq_length * 7 + 1);
        check(ctx, vga_pileup_read(ctx, c.data(), &t.n[0], &t.n[1]));
        t.v = {widen(c, ix_.seq_length * 7)};
        pileup_.add(t);
    }
    const auto t1 = std::chrono::steady_clock::now();
    if (opt_.call_variants && call_now)
        variant_fetch(ctx, variants_, [&](uint64_t cap, uint32_t *pos, uint8_t *gt, uint32_t *qual, uint64_t *iq, uint64_t *depth, uint64_t *counts, uint64_t *nt, uint64_t *nc) {
            return vga_variant_call(ctx, opt_.call_error, opt_.call_min_depth, opt_.call_min_qual, cap, pos, gt, qual, iq, depth, counts, nt, nc);
        });
    if (inserting() && call_now) {  // the sites of the calls just made, from the context's own counters
        const std::vector<uint32_t> pos = insertion_sites();
        InsertionCalls &c = ins_calls_;
        check(ctx, vga_insertion_call(ctx, pos.size(), pos.data(), c.length.data(), c.length_reads.data(), c.seq.data(), c.seq_reads.data(), nullptr));
    } else if (inserting()) {  // the whole table for the sum: 196 bytes per base
        Counters t;
        std::vector<uint32_t> c(ix_.seq_length * IA_COLS + 1);
        check(ctx, vga_insertion_read(ctx, c.data(), &t.n[0], nullptr, &t.n[1]));
        t.v = {widen(c, ix_.seq_length * IA_COLS)};
        insertions_.add(t);
    }
    if (deleting()) {
        DeletionCalls &d = deletions_;
        check(ctx, vga_deletion_read(ctx, nullptr, &d.n_alignments, &d.n_events, &d.n_end_runs));
        if (call_now) {  // from the context's own store and counters
            deletion_fetch(ctx, d, [&](uint64_t cap, uint32_t *first, uint32_t *len, uint32_t *last, uint8_t *state, uint32_t *qual, uint64_t *depth, uint64_t *reads,
                                       uint64_t *nd, uint64_t *nc) {
                return vga_deletion_call(ctx, opt_.call_error, opt_.call_min_depth, opt_.call_min_qual, cap, first, len, last, state, qual, depth, reads, nd, nc);
            });
        } else {  // the whole store for the call on the summed table: 12 bytes per event
            uint64_t n_events = 0;
            d.events.assign(d.n_events * DL_EVENT_WORDS + 1, 0);
            check(ctx, vga_deletion_read(ctx, d.events.data(), nullptr, &n_events, nullptr));
            if (n_events != d.n_events) throw Error("--call-deletions: the store of slot " + std::to_string(slot) + " changed while it was read");
            d.events.resize(n_events * DL_EVENT_WORDS);
        }
    }
    if (phasing() && call_now) {  // the heterozygous sites of the calls just made, from the context's own store
        phase_sites();
        PhaseLinks &p = phase_;
        check(ctx, vga_phase_links(ctx, p.pos.size(), p.pos.data(), p.x.data(), p.y.data(), p.links.data(), p.site_reads.data(), &p.n_reads));
        if (tagging() || joining() || hap_typing()) p.chain(opt_.phase_min_links);
        if (joining())  // the sets of the chain just made; what follows works on the joined ones
            join_fetch(ctx, join_, p, opt_.phase_join_min_reads, [&](uint64_t cap_rows, uint32_t *table, uint64_t *n_sets) {
                return vga_phase_set_links(ctx, p.pos.size(), p.pos.data(), p.x.data(), p.y.data(), p.ps.data(), p.flip.data(), cap_rows, table, n_sets, nullptr);
            });
        if (tagging())
            tags_fetch(ctx, tags_, p.n_reads, [&](uint64_t cap, uint32_t *rows, uint64_t *n_rows) {
                return vga_phase_tags(ctx, p.pos.size(), p.pos.data(), p.x.data(), p.y.data(), sets_ps().data(), sets_flip().data(), cap, rows, n_rows, nullptr);
            });
        if (hap_calling())  // every call just made, under the sets just made
            hap_counts_fetch(ctx, hap_counts_, variants_.n_calls, [&](uint64_t cap, uint32_t *rows, uint64_t *n_rows) {
                return vga_haplotype_counts(ctx, variants_.n_calls, variants_.pos.data(), p.pos.size(), p.pos.data(), p.x.data(), p.y.data(), sets_ps().data(),
                                            sets_flip().data(), cap, rows, n_rows, nullptr);
            });
        if (hap_typing()) {  // the rows beside the store just linked, under the sets just made
            HapPaths &h = hap_paths_;
            uint64_t n_rows = 0;
            check(ctx, vga_haplotype_paths_store(ctx, nullptr, nullptr, &n_rows, nullptr));
            h.scored.assign(n_rows + 1, 0);
            check(ctx, vga_haplotype_paths_store(ctx, nullptr, h.scored.data(), &n_rows, nullptr));
            h.n_scored = 0;
            for (uint64_t r = 0; r < n_rows; r++) h.n_scored += h.scored[r];
            hap_paths_fetch(ctx, h, sets_ps(), p.pos.size(), np, [&](uint64_t cap_groups, uint64_t *reads, uint64_t *table, uint64_t *n_sets) {
                return vga_haplotype_paths(ctx, p.pos.size(), p.pos.data(), p.x.data(), p.y.data(), sets_ps().data(), sets_flip().data(), cap_groups, reads, table, n_sets,
                                           nullptr);
            });
        }
    } else if (phasing()) {  // the whole store: the context may be gone before the summed call
        PhaseStore s;
        uint64_t n_reads = 0, n_words = 0;
        check(ctx, vga_phase_read(ctx, nullptr, nullptr, &n_reads, &n_words));
        s.recs.resize(n_reads * 3 + 1); s.words.resize(n_words + 1);
        check(ctx, vga_phase_read(ctx, s.recs.data(), s.words.data(), &n_reads, &n_words));
        s.recs.resize(n_reads * 3); s.words.resize(n_words);
        if (tagging() && tags_.read_ids.size() != n_reads)
            throw Error("--haplotag: the phase store of slot " + std::to_string(slot) + " holds " + std::to_string(n_reads) + " reads, and " +
                        std::to_string(tags_.read_ids.size()) + " reads were noted as kept");
        phase_store_.add(s);
        if (hap_typing()) {  // the deficit rows beside it, in the same order
            uint64_t n_rows = 0;
            uint32_t paths = 0;
            check(ctx, vga_haplotype_paths_store(ctx, nullptr, nullptr, &n_rows, &paths));
            if (n_rows != n_reads || paths != np)
                throw Error("--haplotype-paths: the deficit store of slot " + std::to_string(slot) + " holds " + std::to_string(n_rows) + " rows of " + std::to_string(paths) +
                            " paths, and its phase store " + std::to_string(n_reads) + " reads");
            std::vector<uint8_t> d(n_rows * np + 1), sc(n_rows + 1);
            check(ctx, vga_haplotype_paths_store(ctx, d.data(), sc.data(), &n_rows, &paths));
            hap_paths_.deficits.insert(hap_paths_.deficits.end(), d.begin(), d.begin() + (long)(n_rows * np));
            hap_paths_.scored.insert(hap_paths_.scored.end(), sc.begin(), sc.begin() + (long)n_rows);
        }
    }
    if (piling() && getenv("VGA_TRACE"))
        fprintf(stderr, "[vgh-trace] slot %u: pileup table read in %.3f ms, variants called in %.3f ms\n", slot,
                std::chrono::duration<double, std::milli>(t1 - t0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
}

void Tables::end(vga_ctx *ctx) const
{
    if (coverage()) (void)vga_coverage_end(ctx);
    if (scoring()) (void)vga_path_support_end(ctx);  // (and genotyping, the edit distance and the store of the path abundance with it)
    if (hap_typing()) (void)vga_haplotype_paths_end(ctx);
    if (phasing()) (void)vga_phase_end(ctx);
    if (deleting()) (void)vga_deletion_end(ctx);
    if (piling()) (void)vga_pileup_end(ctx);
    if (inserting()) (void)vga_insertion_end(ctx);
}

void Tables::add(const Tables &o)
{
    coverage_.add(o.coverage_);
    paths_.add(o.paths_);
    pairs_.add(o.pairs_);
    costs_.add(o.costs_);
    edit_.add(o.edit_);
    pileup_.add(o.pileup_);
    insertions_.add(o.insertions_);
    deletions_.events.insert(deletions_.events.end(), o.deletions_.events.begin(), o.deletions_.events.end());  // (the call does not depend on the order)
    deletions_.n_alignments += o.deletions_.n_alignments; deletions_.n_events += o.deletions_.n_events; deletions_.n_end_runs += o.deletions_.n_end_runs;
    phase_store_.add(o.phase_store_);
    hap_paths_.deficits.insert(hap_paths_.deficits.end(), o.hap_paths_.deficits.begin(), o.hap_paths_.deficits.end());  // (in the order of the records)
    hap_paths_.scored.insert(hap_paths_.scored.end(), o.hap_paths_.scored.begin(), o.hap_paths_.scored.end());
    tags_.read_ids.insert(tags_.read_ids.end(), o.tags_.read_ids.begin(), o.tags_.read_ids.end());  // (in the order of the records)
    abundance_.deficits.insert(abundance_.deficits.end(), o.abundance_.deficits.begin(), o.abundance_.deficits.end());  // (the estimate does not depend on the order)
    abundance_.scored.insert(abundance_.scored.end(), o.abundance_.scored.begin(), o.abundance_.scored.end());
    abundance_.n_kept += o.abundance_.n_kept;
}

void Tables::phase_sites()
{
    PhaseLinks &p = phase_;
    p.pos.clear(); p.x.clear(); p.y.clear();
    for (uint64_t j = 0; j < variants_.n_calls; j++) {
        const uint8_t x = variants_.gt[j] & 7u, y = (variants_.gt[j] >> 3) & 7u;
        if (x < y) { p.pos.push_back(variants_.pos[j]); p.x.push_back(x); p.y.push_back(y); }
    }
    const size_t n = p.pos.size();
    p.links.assign((n + 1) * PH_LINK_ROW, 0); p.site_reads.assign((n + 1) * PH_SITE_COLS, 0);
    p.pos.reserve(n + 1); p.x.reserve(n + 1); p.y.reserve(n + 1);
}

std::vector<uint32_t> Tables::insertion_sites()
{
    std::vector<uint32_t> pos;
    InsertionCalls &c = ins_calls_;
    c.site.clear();
    for (uint64_t j = 0; j < variants_.n_calls; j++)
        if ((variants_.gt[j] >> 6) == 1u || (variants_.gt[j] >> 6) == 2u) { c.site.push_back(j); pos.push_back(variants_.pos[j]); }
    const size_t n = pos.size();
    c.length.assign(n + 1, 0); c.length_reads.assign(n + 1, 0); c.seq.assign((n + 1) * IA_MAX_LEN, 0); c.seq_reads.assign((n + 1) * IA_MAX_LEN, 0);
    pos.reserve(n + 1);
    return pos;
}

void Tables::call(vga_ctx *ctx)
{
    if (abundance()) {
        Abundance &a = abundance_;
        const size_t np = opt_.paths.n_paths();
        if (a.scored.size() != a.n_kept || a.deficits.size() != a.n_kept * np)
            throw Error("--path-abundance: the contexts kept " + std::to_string(a.n_kept) + " rows and handed over " + std::to_string(a.scored.size()));
        a.theta.assign(np + 1, 0); a.reads_q16.assign(np + 1, 0); a.best.assign(np + 1, 0);
        a.deficits.push_back(0); a.scored.push_back(0);  // (never a null array)
        check(ctx, vga_path_abundance_rows(ctx, a.n_kept, (uint32_t)np, a.deficits.data(), a.scored.data(), opt_.abundance_lambda, opt_.abundance_iters,
                                           opt_.abundance_tol, a.theta.data(), a.reads_q16.data(), a.best.data(), &a.n_scored, &a.iterations, &a.converged));
        trace_mark("path abundance estimated");
    }
    if (!opt_.call_variants) return;
    pileup_.pad({ix_.seq_length * 7});
    variant_fetch(ctx, variants_, [&](uint64_t cap, uint32_t *pos, uint8_t *gt, uint32_t *qual, uint64_t *iq, uint64_t *depth, uint64_t *counts, uint64_t *nt, uint64_t *nc) {
        return vga_variant_call_table(ctx, ix_.seq_length, pileup_.v[0].data(), ix_.seq_fwd.data(), opt_.call_error, opt_.call_min_depth, opt_.call_min_qual, cap,
                                      pos, gt, qual, iq, depth, counts, nt, nc);
    });
    trace_mark("variants called");
    if (deleting()) {  // the concatenated stores against the summed pileup table
        DeletionCalls &d = deletions_;
        if (d.events.size() != d.n_events * DL_EVENT_WORDS)
            throw Error("--call-deletions: the contexts kept " + std::to_string(d.n_events) + " events and handed over " + std::to_string(d.events.size() / DL_EVENT_WORDS));
        d.events.push_back(0);  // (never a null array)
        deletion_fetch(ctx, d, [&](uint64_t cap, uint32_t *first, uint32_t *len, uint32_t *last, uint8_t *state, uint32_t *qual, uint64_t *depth, uint64_t *reads,
                                   uint64_t *nd, uint64_t *nc) {
            return vga_deletion_call_table(ctx, d.n_events, d.events.data(), ix_.seq_length, pileup_.v[0].data(), opt_.call_error, opt_.call_min_depth,
                                           opt_.call_min_qual, cap, first, len, last, state, qual, depth, reads, nd, nc);
        });
        trace_mark("deletions called");
    }
    if (phasing()) {
        phase_sites();
        PhaseLinks &p = phase_;
        std::vector<uint8_t> ref(p.pos.size() + 1);
        for (size_t h = 0; h < p.pos.size(); h++) ref[h] = ph_ref_of(ix_.seq_fwd[p.pos[h]]);
        const PhaseStore &s = phase_store_;
        p.n_reads = s.recs.size() / 3;
        check(ctx, vga_phase_links_lists(ctx, ix_.seq_length, p.n_reads, s.recs.data(), s.words.size(), s.words.data(), p.pos.size(), p.pos.data(), p.x.data(),
                                         p.y.data(), ref.data(), p.links.data(), p.site_reads.data()));
        trace_mark("phase links counted");
        if (tagging() || joining() || hap_typing()) p.chain(opt_.phase_min_links);
        if (joining()) {
            join_fetch(ctx, join_, p, opt_.phase_join_min_reads, [&](uint64_t cap_rows, uint32_t *table, uint64_t *n_sets) {
                return vga_phase_set_links_lists(ctx, ix_.seq_length, p.n_reads, s.recs.data(), s.words.size(), s.words.data(), p.pos.size(), p.pos.data(), p.x.data(),
                                                 p.y.data(), ref.data(), p.ps.data(), p.flip.data(), cap_rows, table, n_sets);
            });
            trace_mark("phase sets joined");
        }
        if (tagging()) {
            tags_fetch(ctx, tags_, p.n_reads, [&](uint64_t cap, uint32_t *rows, uint64_t *n_rows) {
                return vga_phase_tags_lists(ctx, ix_.seq_length, p.n_reads, s.recs.data(), s.words.size(), s.words.data(), p.pos.size(), p.pos.data(), p.x.data(),
                                            p.y.data(), ref.data(), sets_ps().data(), sets_flip().data(), cap, rows, n_rows);
            });
            trace_mark("reads tagged");
        }
        if (hap_calling()) {
            std::vector<uint8_t> cref(variants_.n_calls + 1);
            for (uint64_t j = 0; j < variants_.n_calls; j++) cref[j] = ph_ref_of(ix_.seq_fwd[variants_.pos[j]]);
            hap_counts_fetch(ctx, hap_counts_, variants_.n_calls, [&](uint64_t cap, uint32_t *rows, uint64_t *n_rows) {
                return vga_haplotype_counts_lists(ctx, ix_.seq_length, p.n_reads, s.recs.data(), s.words.size(), s.words.data(), variants_.n_calls,
                                                  variants_.pos.data(), cref.data(), p.pos.size(), p.pos.data(), p.x.data(), p.y.data(), ref.data(), sets_ps().data(),
                                                  sets_flip().data(), cap, rows, n_rows);
            });
            trace_mark("haplotypes counted");
        }
        if (hap_typing()) {
            HapPaths &h = hap_paths_;
            const size_t np = opt_.paths.n_paths();
            if (h.scored.size() != p.n_reads || h.deficits.size() != p.n_reads * np)
                throw Error("--haplotype-paths: the contexts kept " + std::to_string(p.n_reads) + " reads and " + std::to_string(h.scored.size()) + " deficit rows");
            h.n_scored = 0;
            for (uint8_t v : h.scored) h.n_scored += v;
            h.deficits.push_back(0); h.scored.push_back(0);  // (never a null array)
            hap_paths_fetch(ctx, h, sets_ps(), p.pos.size(), np, [&](uint64_t cap_groups, uint64_t *reads, uint64_t *table, uint64_t *n_sets) {
                return vga_haplotype_paths_lists(ctx, ix_.seq_length, p.n_reads, s.recs.data(), s.words.size(), s.words.data(), (uint32_t)np, h.deficits.data(),
                                                 h.scored.data(), p.pos.size(), p.pos.data(), p.x.data(), p.y.data(), ref.data(), sets_ps().data(), sets_flip().data(),
                                                 cap_groups, reads, table, n_sets);
            });
            trace_mark("haplotype paths summed");
        }
    }
    if (!inserting()) return;
    insertions_.pad({ix_.seq_length * IA_COLS});
    const std::vector<uint32_t> pos = insertion_sites();
    std::vector<uint64_t> rows(pos.size() * IA_COLS + 1);
    for (size_t s = 0; s < pos.size(); s++)
        std::copy_n(insertions_.v[0].begin() + (long)((uint64_t)pos[s] * IA_COLS), IA_COLS, rows.begin() + (long)(s * IA_COLS));
    InsertionCalls &c = ins_calls_;
    check(ctx, vga_insertion_call_table(ctx, pos.size(), rows.data(), c.length.data(), c.length_reads.data(), c.seq.data(), c.seq_reads.data(), nullptr));
    trace_mark("insertions called");
}

void Tables::write(MapOutput &out, const ReadRows &rows, const std::string &out_prefix)
{
    const size_t np = opt_.paths.n_paths(), n_pairs = vga_pair_count(np);
    const bool files = !out_prefix.empty();
    if (coverage()) {
        coverage_.pad({ix_.seq_length, ix_.n_nodes, ix_.n_edges});
        out.n_coverage = coverage_.n[0];
        if (files) coverage_write(ix_, coverage_, out_prefix);
        trace_mark("coverage tables written");
    }
    if (opt_.genotype) {
        pairs_.pad({n_pairs, n_pairs, n_pairs, n_pairs});
        genotype_write(opt_, pairs_, out, out_prefix);
        trace_mark("genotype table written");
    }
    if (opt_.genotype_likelihood) {
        costs_.pad({n_pairs});
        likelihood_write(opt_, costs_, out, out_prefix);
        trace_mark("genotype likelihood table written");
    }
    if (edit()) {
        out.n_edit_alignments = edit_.n[0]; out.n_edit_too_long = edit_.n[1];
        if (opt_.path_edit) {
            edit_.pad({np, np, np, np});
            if (files) path_edit_write(ix_, opt_, edit_, rows.edit, out_prefix);
            trace_mark("path edit tables written");
        }
    }
    if (scoring()) {
        out.n_path_scored = paths_.n[0]; out.n_path_unplaced = paths_.n[1];
        if (opt_.path_support) {
            paths_.pad({np, np, np, np});
            if (files) path_support_write(opt_, paths_, rows.path, out_prefix);
            trace_mark("path support tables written");
        }
    }
    if (abundance()) {
        abundance_.theta.resize(np + 1, 0); abundance_.reads_q16.resize(np + 1, 0); abundance_.best.resize(np + 1, 0);
        abundance_write(opt_, abundance_, out, out_prefix);
        trace_mark("path abundance written");
    }
    if (opt_.call_variants) {
        out.n_variant_tested = variants_.n_tested; out.n_variant_calls = variants_.n_calls;
        if (files) variant_write(ix_, variants_, out_prefix);
        trace_mark("variants written");
    }
    if (phasing()) {
        phase_write(ix_, phase_, opt_.phase_min_links, out, out_prefix);
        trace_mark("phase written");
        if (joining()) {
            phase_join_write(ix_, phase_, join_, out, out_prefix);
            trace_mark("phase join written");
        }
        if (tagging()) {
            haplotag_write(tags_, out, out_prefix);
            trace_mark("haplotags written");
        }
        if (hap_calling()) {
            haplotype_calls_write(ix_, variants_, hap_counts_, out, out_prefix);
            trace_mark("haplotype calls written");
        }
        if (hap_typing()) {
            haplotype_paths_write(opt_, sets_ps(), phase_.pos.size(), hap_paths_, phase_.n_reads, out, out_prefix);
            trace_mark("haplotype paths written");
        }
    }
    if (inserting()) {
        insertion_write(ix_, variants_, ins_calls_, out, out_prefix);
        trace_mark("insertions written");
    }
    if (deleting()) {
        deletion_write(ix_, deletions_, out, out_prefix);
        trace_mark("deletions written");
    }
    if (opt_.pileup) {
        pileup_.pad({ix_.seq_length * 7});
        out.n_pileup = pileup_.n[0]; out.n_leading_ins = pileup_.n[1];
        if (files) pileup_write(ix_, pileup_, out_prefix);
        trace_mark("pileup table written");
    }
}

}  // namespace vgh
