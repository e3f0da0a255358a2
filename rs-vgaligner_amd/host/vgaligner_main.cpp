// vgaligner_main.cpp -- `vgaligner index` / `vgaligner map`: same flags, defaults and output naming as the
// reference CLI (src/subcommands/cli.yml:1-175, index_main.rs:11-87, map_main.rs:12-118).
#include "vgh.hpp"

#include <cstdio>
#include <malloc.h>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <unistd.h>

using namespace vgh;

namespace {

// short flag, long flag (src/subcommands/cli.yml), takes a value, key (the argument's name in cli.yml)
struct Flag { const char *shortf, *longf; bool takes_value; const char *key; };

const Flag INDEX_FLAGS[] = {{"-i", "--input", true, "input"}, {"-o", "--output", true, "out-prefix"}, {"-k", "--kmer-length", true, "kmer-length"},
                            {"-e", "--max-furcations", true, "max-furcations"}, {"-m", "--max-degree", true, "max-degree"},
                            {"-r", "--sampling-rate", true, "sampling-rate"}, {"-g", "--generate-mappings", false, "generate-mappings"},
                            {"-p", "--mappings-path", true, "mappings-path"}, {"-t", "--threads", true, "n-threads"},
                            // the argument names, accepted as long flags too
                            {"", "--out-prefix", true, "out-prefix"}, {"", "--n-threads", true, "n-threads"},
                            // not in the reference: build the k-mer half of the index on this GPU (vga_index_build_kmers)
                            {"-d", "--device", true, "device"}};
const Flag MAP_FLAGS[] = {{"-i", "--index", true, "index"}, {"-f", "--input-file", true, "input-file"}, {"-o", "--out", true, "out-prefix"},
                          {"-g", "--max-gap-length", true, "max-gap-length"}, {"-r", "--max-mismatch-rate", true, "max-mismatch-rate"},
                          {"-c", "--chain-overlap-max", true, "chain-overlap-max"}, {"-a", "--chain-min-anchors", true, "chain-min-anchors"},
                          {"-b", "--align-best-n", true, "align-best-n"}, {"-C", "--write-console", false, "write-console"},
                          {"-D", "--also-align", false, "also-align"}, {"-t", "--threads", true, "n-threads"},
                          {"-v", "--also-validate", false, "also-validate"}, {"-G", "--graph", true, "graph"},
                          {"-P", "--validation-path", true, "validation-path"}, {"-p", "--poa-aligner", true, "poa-aligner"},
                          {"", "--out-prefix", true, "out-prefix"}, {"", "--n-threads", true, "n-threads"},
                          // not in the reference: --device one GPU, --devices a list (one context + host thread each; an id may
                          // repeat; --devices all: every visible GPU; default: --device 0), --chunk-reads reads per batch (bounded memory; 0 = one batch)
                          {"-d", "--device", true, "device"}, {"", "--devices", true, "devices"}, {"", "--chunk-reads", true, "chunk-reads"},
                          {"", "--poa-remain", true, "poa-remain"},
                          // not in the reference: map each read and its reverse complement, keep the orientation that chains better
                          {"", "--both-strands", false, "both-strands"},
                          // not in the reference: read coverage of bases, nodes and edges, counted on the GPU (three TSV files);
                          // --coverage-only leaves the alignments GAF unwritten
                          {"", "--coverage", false, "coverage"}, {"", "--coverage-only", false, "coverage-only"},
                          // not in the reference: every reported alignment scored against the P lines of --graph on the GPU (two TSV files)
                          {"", "--path-support", false, "path-support"},
                          // not in the reference: read alleles, deletions and insertions per graph base, counted on the GPU (one TSV file)
                          {"", "--pileup", false, "pileup"},
                          // not in the reference: the pairs of P lines of --graph ranked by how well they explain the alignments, added up
                          // on the GPU (one TSV file); --genotype-top N: the best N pairs (20), 0 = all
                          {"", "--genotype", false, "genotype"}, {"", "--genotype-top", true, "genotype-top"},
                          // not in the reference: the pairs of P lines of --graph ranked by the diploid read likelihood, added up on the
                          // GPU (one TSV file); --genotype-lambda N: the cost of one unit of deficit in 1/256 bit (512, 1..4096);
                          // --genotype-cap N: the largest deficit told apart (64, 1..255); --genotype-top applies to it too
                          {"", "--genotype-likelihood", false, "genotype-likelihood"}, {"", "--genotype-lambda", true, "genotype-lambda"},
                          {"", "--genotype-cap", true, "genotype-cap"},
                          // not in the reference: the read of every reported alignment scored against the P lines of --graph by edit
                          // distance on the GPU (two TSV files); --genotype-from edit|support: which of the two scorings the
                          // likelihood reads (support)
                          {"", "--path-edit", false, "path-edit"}, {"", "--genotype-from", true, "genotype-from"},
                          // not in the reference: a diploid call at every graph base from the pileup counters, made on the GPU (one TSV
                          // file with the bases where the reads disagree with the graph); --call-error N: the cost of an observation
                          // neither allele explains in 1/256 bit (1280, 257..8192); --call-min-depth N: the depth from which a base is
                          // tested (4, at least 1); --call-min-qual N: the margin from which a call is reported (512)
                          {"", "--call-variants", false, "call-variants"}, {"", "--call-error", true, "call-error"},
                          {"", "--call-min-depth", true, "call-min-depth"}, {"", "--call-min-qual", true, "call-min-qual"},
                          // not in the reference: length and letters of what the reads insert at the sites --call-variants reports
                          // with an insertion, counted and called on the GPU (one TSV file)
                          {"", "--call-insertions", false, "call-insertions"},
                          // not in the reference (needs --call-variants): every run of deleted graph bases as one event, sorted, counted and
                          // called on the GPU (one TSV file)
                          {"", "--call-deletions", false, "call-deletions"},
                          // not in the reference: the read-backed links between the heterozygous sites --call-variants reports,
                          // counted on the GPU, and the phase chain on them (one TSV file); --phase-min-links N: the reads by which
                          // cis and trans must differ for a link to join two sites (2, 1..65535)
                          {"", "--phase", false, "phase"}, {"", "--phase-min-links", true, "phase-min-links"},
                          // not in the reference: which kept reads go with which haplotype of which phase set of --phase, counted
                          // on the GPU (one TSV file, a row per read and set)
                          {"", "--haplotag", false, "haplotag"},
                          // not in the reference: what the reads tagged a and the reads tagged b of each phase set show at every
                          // reported call inside the set's span, counted on the GPU, and a haploid call on each (one TSV file)
                          {"", "--haplotype-calls", false, "haplotype-calls"},
                          // not in the reference: the phase sets of --phase joined by the reads that are tagged in two of them,
                          // counted on the GPU (three TSV files; --haplotag and --haplotype-calls then work on the joined sets);
                          // --phase-join-min-reads N: the reads by which cis and trans must differ for a link (2, 1..65535)
                          {"", "--phase-join", false, "phase-join"}, {"", "--phase-join-min-reads", true, "phase-join-min-reads"},
                          // --haplotype-paths (with --phase): a haploid ranking of the P lines of --graph for each haplotype of
                          // each phase set, from that haplotype's own reads, summed on the GPU (<out>-haplotype-paths.tsv);
                          // --haplotype-paths-cap C: the largest deficit told apart (64, 1..255); --haplotype-paths-top N: the
                          // paths written per group (5, 0 for all); --haplotype-paths-from support|edit: the matrices scored
                          {"", "--haplotype-paths", false, "haplotype-paths"}, {"", "--haplotype-paths-cap", true, "haplotype-paths-cap"},
                          {"", "--haplotype-paths-top", true, "haplotype-paths-top"}, {"", "--haplotype-paths-from", true, "haplotype-paths-from"},
                          // not in the reference: the share of the reads that each P line of --graph explains, fitted over all paths at
                          // once by expectation-maximisation on the GPU (<out>-path-abundance.tsv); --abundance-lambda N: the cost of one
                          // unit of deficit in 1/256 bit (512, 1..4096); --abundance-cap C: the largest deficit told apart (64, 1..255);
                          // --abundance-iters N: the most iterations (1000, 1..100000); --abundance-tol N: the largest move of a share,
                          // in units of 2^-24, at which the estimate stops (16, 0..16777216); --abundance-min N: the parts per million
                          // from which a path is written (10000, 0 for every path); --abundance-from support|edit: the matrices scored
                          {"", "--path-abundance", false, "path-abundance"}, {"", "--abundance-lambda", true, "abundance-lambda"},
                          {"", "--abundance-cap", true, "abundance-cap"}, {"", "--abundance-iters", true, "abundance-iters"},
                          {"", "--abundance-tol", true, "abundance-tol"}, {"", "--abundance-min", true, "abundance-min"},
                          {"", "--abundance-from", true, "abundance-from"}};

template <size_t N>
std::map<std::string, std::string> parse(const Flag (&flags)[N], int argc, char **argv, int first)
{
    std::map<std::string, std::string> m;
    for (int i = first; i < argc; i++) {
        const Flag *f = nullptr;
        for (const Flag &c : flags)
            if ((c.shortf[0] && !strcmp(argv[i], c.shortf)) || !strcmp(argv[i], c.longf)) { f = &c; break; }
        if (!f) throw Error(std::string("unknown argument ") + argv[i]);
        if (f->takes_value) {
            if (i + 1 >= argc) throw Error(std::string("missing value for ") + argv[i]);
            m[f->key] = argv[++i];
        } else m[f->key] = "1";
    }
    return m;
}

std::string need(const std::map<std::string, std::string> &m, const char *key)
{
    auto it = m.find(key);
    if (it == m.end()) throw Error(std::string("the required argument --") + key + " was not provided");
    return it->second;
}
std::string opt(const std::map<std::string, std::string> &m, const char *key, const std::string &dflt)
{
    auto it = m.find(key);
    return it == m.end() ? dflt : it->second;
}

int index_main(int argc, char **argv)
{
    auto m = parse(INDEX_FLAGS, argc, argv, 2);
    std::string in = need(m, "input");
    std::string prefix = opt(m, "out-prefix", in.size() > 4 ? in.substr(0, in.size() - 4) : in);  // index_main.rs:16-18
    uint64_t k = std::stoull(need(m, "kmer-length"));
    uint64_t furc = std::stoull(opt(m, "max-furcations", "100")), deg = std::stoull(opt(m, "max-degree", "100"));
    if (m.count("sampling-rate")) throw Error("--sampling-rate depends on ahash's hash values and is not supported");
    if (m.count("generate-mappings")) fprintf(stderr, "[vgaligner] --generate-mappings (debug JSON) is not produced by this build\n");
    Index ix;
    if (m.count("device")) {  // same index, same file: only where the k-mers are enumerated and sorted changes
        const int dev = std::stoi(m["device"]);
        vga_ctx *ctx = nullptr;
        if (int rc = vga_ctx_create(dev, &ctx))
            throw Error("--device " + std::to_string(dev) + ": vga_ctx_create failed (" +
                        (rc == VGA_ERR_NO_DEVICE ? std::string("VGA_ERR_NO_DEVICE: no usable MI355X") : "error " + std::to_string(rc)) +
                        "); the GPU index build has no CPU path");
        try {
            ix = Index::build_on_device(HashGraph::from_gfa(in), k, furc, deg, ctx);
        } catch (...) {
            vga_ctx_destroy(ctx);
            throw;
        }
        vga_ctx_destroy(ctx);
    } else
        ix = Index::build(HashGraph::from_gfa(in), k, furc, deg);
    fprintf(stderr, "[vgaligner] Index with k=%llu built: %llu different kmers, %llu positions\n", (unsigned long long)k,
            (unsigned long long)ix.n_kmers, (unsigned long long)ix.n_kmer_pos);
    bool exact = prefix.size() >= 4 && prefix.compare(prefix.size() - 4, 4, ".idx") == 0;  // index.rs:267-278
    ix.store(exact ? prefix : prefix + ".idx");
    return 0;
}

int map_main(int argc, char **argv)
{
    auto m = parse(MAP_FLAGS, argc, argv, 2);
    std::string idx = need(m, "index"), in = need(m, "input-file");
    std::string dflt_prefix;  // map_main.rs:19-28 (strips 3 chars for ...fa / ...fasta, else 4)
    auto ends = [&](const char *s) { size_t n = strlen(s); return in.size() >= n && in.compare(in.size() - n, n, s) == 0; };
    dflt_prefix = (ends("fa") || ends("fasta")) ? in.substr(0, in.size() - 3) : in.substr(0, in.size() > 4 ? in.size() - 4 : 0);
    MapOptions o;
    std::string prefix = opt(m, "out-prefix", dflt_prefix);
    o.max_gap = std::stoull(opt(m, "max-gap-length", "1000"));
    o.max_mismatch_rate = std::stod(opt(m, "max-mismatch-rate", "0.1"));
    o.chain_min_n_anchors = std::stoull(opt(m, "chain-min-anchors", "3"));
    o.align_best_n = std::stoull(opt(m, "align-best-n", "1"));
    o.write_console = m.count("write-console") > 0;
    o.also_align = m.count("also-align") > 0;
    o.poa_aligner = need(m, "poa-aligner");  // cli.yml:169-175: required
    o.device = std::stoi(opt(m, "device", "0"));
    if (m.count("poa-remain")) {  // which path the adaptive band's `remain` follows (include/vga_hip.h: VGA_REMAIN_*)
        const std::string r = m["poa-remain"];
        if (r == "longest") o.poa_remain_rule = VGA_REMAIN_LONGEST_PATH;
        else if (r == "first-edge") o.poa_remain_rule = VGA_REMAIN_FIRST_OUT_EDGE;
        else throw Error("--poa-remain takes longest or first-edge");
    }
    o.both_strands = m.count("both-strands") > 0;
    o.coverage_only = m.count("coverage-only") > 0;
    o.coverage = o.coverage_only || m.count("coverage") > 0;
    if (o.coverage && !o.also_align) throw Error(std::string(o.coverage_only ? "--coverage-only" : "--coverage") + " counts alignments: it needs --also-align");
    o.path_support = m.count("path-support") > 0;
    if (o.path_support && !o.also_align) throw Error("--path-support scores alignments: it needs --also-align");
    o.pileup = m.count("pileup") > 0;
    if (o.pileup && !o.also_align) throw Error("--pileup counts alignments: it needs --also-align");
    o.genotype = m.count("genotype") > 0;
    if (o.genotype && !o.also_align) throw Error("--genotype calls from alignments: it needs --also-align");
    o.genotype_likelihood = m.count("genotype-likelihood") > 0;
    if (o.genotype_likelihood && !o.also_align) throw Error("--genotype-likelihood calls from alignments: it needs --also-align");
    if (m.count("genotype-top")) {
        const std::string v = m["genotype-top"];
        if (v.empty() || v.size() > 18 || v.find_first_not_of("0123456789") != std::string::npos)
            throw Error("--genotype-top takes a number of pairs, 0 for all: not " + v);
        if (!o.genotype && !o.genotype_likelihood) throw Error("--genotype-top has no meaning without --genotype or --genotype-likelihood");
        o.genotype_top = std::stoull(v);
    }
    // --genotype-lambda, --genotype-cap: a number inside the range of vga_genotype_lik_begin, and only beside --genotype-likelihood
    auto likelihood_value = [&](const char *key, uint32_t lo, uint32_t hi, uint32_t &into) {
        if (!m.count(key)) return;
        const std::string v = m[key], flag = std::string("--") + key;
        if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos || std::stoul(v) < lo || std::stoul(v) > hi)
            throw Error(flag + " takes a number from " + std::to_string(lo) + " to " + std::to_string(hi) + ": not " + v);
        if (!o.genotype_likelihood) throw Error(flag + " has no meaning without --genotype-likelihood");
        into = (uint32_t)std::stoul(v);
    };
    likelihood_value("genotype-lambda", 1, 4096, o.genotype_lambda);
    likelihood_value("genotype-cap", 1, 255, o.genotype_cap);
    o.path_edit = m.count("path-edit") > 0;
    if (o.path_edit && !o.also_align) throw Error("--path-edit scores alignments: it needs --also-align");
    if (m.count("genotype-from")) {
        const std::string v = m["genotype-from"];
        if (v != "edit" && v != "support") throw Error("--genotype-from takes edit or support: not " + v);
        if (!o.genotype_likelihood) throw Error("--genotype-from has no meaning without --genotype-likelihood");
        o.genotype_from_edit = v == "edit";
    }
    o.call_variants = m.count("call-variants") > 0;
    if (o.call_variants && !o.also_align) throw Error("--call-variants calls from alignments: it needs --also-align");
    // --call-error, --call-min-depth, --call-min-qual: a number inside the range of vga_variant_call, and only beside --call-variants
    auto call_value = [&](const char *key, uint64_t lo, uint64_t hi, uint64_t &into) {
        if (!m.count(key)) return;
        const std::string v = m[key], flag = std::string("--") + key;
        if (v.empty() || v.size() > 18 || v.find_first_not_of("0123456789") != std::string::npos || std::stoull(v) < lo || std::stoull(v) > hi)
            throw Error(flag + " takes a number " + (hi == UINT64_MAX ? "of at least " + std::to_string(lo) : "from " + std::to_string(lo) + " to " + std::to_string(hi)) + ": not " + v);
        if (!o.call_variants) throw Error(flag + " has no meaning without --call-variants");
        into = std::stoull(v);
    };
    uint64_t call_error = o.call_error;
    call_value("call-error", 257, 8192, call_error);
    o.call_error = (uint32_t)call_error;
    call_value("call-min-depth", 1, UINT64_MAX, o.call_min_depth);
    call_value("call-min-qual", 0, UINT64_MAX, o.call_min_qual);
    o.call_insertions = m.count("call-insertions") > 0;
    if (o.call_insertions && !o.also_align) throw Error("--call-insertions calls from alignments: it needs --also-align");
    if (o.call_insertions && !o.call_variants) throw Error("--call-insertions calls at the sites of --call-variants: it needs --call-variants");
    o.call_deletions = m.count("call-deletions") > 0;
    if (o.call_deletions && !o.also_align) throw Error("--call-deletions calls from alignments: it needs --also-align");
    if (o.call_deletions && !o.call_variants) throw Error("--call-deletions calls with the depth and the parameters of --call-variants: it needs --call-variants");
    o.phase = m.count("phase") > 0;
    if (o.phase && !o.call_variants) throw Error("--phase links the heterozygous sites of --call-variants: it needs --call-variants");
    if (m.count("phase-min-links")) {
        const std::string v = m["phase-min-links"];
        if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos || std::stoul(v) < 1 || std::stoul(v) > 65535)
            throw Error("--phase-min-links takes a number from 1 to 65535: not " + v);
        if (!o.phase) throw Error("--phase-min-links has no meaning without --phase");
        o.phase_min_links = (uint32_t)std::stoul(v);
    }
    o.haplotag = m.count("haplotag") > 0;
    if (o.haplotag && !o.phase) throw Error("--haplotag assigns reads to the haplotypes of the phase sets of --phase: it needs --phase");
    o.haplotype_calls = m.count("haplotype-calls") > 0;
    if (o.haplotype_calls && !o.haplotag) throw Error("--haplotype-calls counts what the reads tagged by --haplotag show: it needs --haplotag");
    o.phase_join = m.count("phase-join") > 0;
    if (o.phase_join && !o.phase) throw Error("--phase-join joins the phase sets of --phase: it needs --phase");
    if (m.count("phase-join-min-reads")) {
        const std::string v = m["phase-join-min-reads"];
        if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos || std::stoul(v) < 1 || std::stoul(v) > 65535)
            throw Error("--phase-join-min-reads takes a number from 1 to 65535: not " + v);
        if (!o.phase_join) throw Error("--phase-join-min-reads has no meaning without --phase-join");
        o.phase_join_min_reads = (uint32_t)std::stoul(v);
    }
    o.haplotype_paths = m.count("haplotype-paths") > 0;
    if (o.haplotype_paths && !o.phase) throw Error("--haplotype-paths types the haplotypes of the phase sets of --phase: it needs --phase");
    for (const char *key : {"haplotype-paths-cap", "haplotype-paths-top", "haplotype-paths-from"})
        if (m.count(key) && !o.haplotype_paths) throw Error(std::string("--") + key + " has no meaning without --haplotype-paths");
    if (m.count("haplotype-paths-cap")) {
        const std::string v = m["haplotype-paths-cap"];
        if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos || std::stoul(v) < 1 || std::stoul(v) > 255)
            throw Error("--haplotype-paths-cap takes a number from 1 to 255: not " + v);
        o.haplotype_paths_cap = (uint32_t)std::stoul(v);
    }
    if (m.count("haplotype-paths-top")) {
        const std::string v = m["haplotype-paths-top"];
        if (v.empty() || v.size() > 18 || v.find_first_not_of("0123456789") != std::string::npos)
            throw Error("--haplotype-paths-top takes a number of paths, 0 for all: not " + v);
        o.haplotype_paths_top = std::stoull(v);
    }
    if (m.count("haplotype-paths-from")) {
        const std::string v = m["haplotype-paths-from"];
        if (v != "edit" && v != "support") throw Error("--haplotype-paths-from takes edit or support: not " + v);
        o.haplotype_paths_from_edit = v == "edit";
    }
    o.path_abundance = m.count("path-abundance") > 0;
    if (o.path_abundance && !o.also_align) throw Error("--path-abundance estimates from alignments: it needs --also-align");
    for (const char *key : {"abundance-lambda", "abundance-cap", "abundance-iters", "abundance-tol", "abundance-min", "abundance-from"})
        if (m.count(key) && !o.path_abundance) throw Error(std::string("--") + key + " has no meaning without --path-abundance");
    auto abundance_value = [&](const char *key, uint64_t lo, uint64_t hi) -> uint64_t {
        const std::string v = m[key], flag = std::string("--") + key;
        if (v.empty() || v.size() > 18 || v.find_first_not_of("0123456789") != std::string::npos || std::stoull(v) < lo || std::stoull(v) > hi)
            throw Error(flag + " takes a number " + (hi == UINT64_MAX ? "of at least " + std::to_string(lo) : "from " + std::to_string(lo) + " to " + std::to_string(hi)) + ": not " + v);
        return std::stoull(v);
    };
    if (m.count("abundance-lambda")) o.abundance_lambda = (uint32_t)abundance_value("abundance-lambda", 1, 4096);
    if (m.count("abundance-cap")) o.abundance_cap = (uint32_t)abundance_value("abundance-cap", 1, 255);
    if (m.count("abundance-iters")) o.abundance_iters = (uint32_t)abundance_value("abundance-iters", 1, 100000);
    if (m.count("abundance-tol")) o.abundance_tol = (uint32_t)abundance_value("abundance-tol", 0, 1u << 24);
    if (m.count("abundance-min")) o.abundance_min = abundance_value("abundance-min", 0, UINT64_MAX);
    if (m.count("abundance-from")) {
        const std::string v = m["abundance-from"];
        if (v != "edit" && v != "support") throw Error("--abundance-from takes edit or support: not " + v);
        o.abundance_from_edit = v == "edit";
    }
    o.also_validate = m.count("also-validate") > 0;
    if (o.also_validate) {
        if (!o.also_align) fprintf(stderr, "[vgaligner] --also-validate has no effect without --also-align (map.rs:150-186)\n");
        o.validation_path = need(m, "validation-path");  // map.rs:201 unwraps it
    }
    if (o.also_align && !m.count("graph")) throw Error("--also-align needs --graph (the reference unwraps it, map.rs:157)");
    bool exact = idx.size() >= 4 && idx.compare(idx.size() - 4, 4, ".idx") == 0;
    trace_mark("start");
    if (m.count("devices") && m["devices"] == "all") o.all_devices = true;
    else if (m.count("devices")) {
        const std::string l = m["devices"];
        size_t p0 = 0;
        while (p0 <= l.size()) {
            const size_t p1 = l.find(',', p0);
            const std::string tok = l.substr(p0, p1 == std::string::npos ? std::string::npos : p1 - p0);
            if (!tok.empty()) o.devices.push_back(std::stoi(tok));
            if (p1 == std::string::npos) break;
            p0 = p1 + 1;
        }
        if (o.devices.empty()) throw Error("--devices needs a comma-separated list of GPU ids");
    }
    // --path-support, --genotype, --genotype-likelihood, --path-edit, --haplotype-paths, --path-abundance: the P lines of --graph, and the graph checked against the index,
    // before any device is opened
    std::unique_ptr<HashGraph> graph;
    const bool scoring = scoring_on(o);
    if (scoring) {
        graph.reset(new HashGraph(HashGraph::from_gfa(m["graph"])));
        o.paths = path_table(*graph);
        if (o.paths.n_paths() == 0) throw Error(std::string(o.path_support ? "--path-support: " : o.genotype ? "--genotype: " : o.genotype_likelihood ? "--genotype-likelihood: " : o.path_edit ? "--path-edit: " : o.haplotype_paths ? "--haplotype-paths: " : "--path-abundance: ") + m["graph"] + " has no P line");
    } else
        prewarm_contexts(o);  // (HIP starts beside the reading of the index and the reads)
    Index ix = Index::load(exact ? idx : idx + ".idx");
    if (scoring) {
        check_graph_matches_index(*graph, ix);
        graph.reset();
        prewarm_contexts(o);
    }
    trace_mark("index loaded");
    std::vector<QuerySequence> reads = read_seqs_from_file(in);
    trace_mark("reads parsed");
    fprintf(stderr, "[vgaligner] Found %zu reads!\n", reads.size());
    o.leave_contexts = !getenv("VGA_NO_FAST_EXIT");
    o.chunk_reads = std::stoull(opt(m, "chunk-reads", "32768"));
    o.keep_text = o.write_console || o.also_validate;
    MapOutput out = map_reads_multi(ix, reads, o, prefix);
    fprintf(stderr, "[vgaligner] %llu GPU context(s), %llu batch(es)\n", (unsigned long long)out.n_devices, (unsigned long long)out.n_chunks);
    fprintf(stderr, "[vgaligner] Chaining took: %.0f ms\n", out.ms_map);
    if (o.both_strands)
        fprintf(stderr, "[vgaligner] %llu of %llu reads on the reverse strand\n", (unsigned long long)out.n_reverse, (unsigned long long)out.n_reads);
    if (o.also_align) fprintf(stderr, "[vgaligner] Alignment took: %.0f ms; Found %llu alignments!\n", out.ms_align, (unsigned long long)out.n_reads);
    if (o.coverage) fprintf(stderr, "[vgaligner] Coverage: %llu alignments counted\n", (unsigned long long)out.n_coverage);
    if (o.path_support)
        fprintf(stderr, "[vgaligner] Path support: %llu alignments scored, %llu unplaced\n", (unsigned long long)out.n_path_scored,
                (unsigned long long)out.n_path_unplaced);
    if (o.genotype) {
        if (out.n_genotype_pairs)
            fprintf(stderr, "[vgaligner] genotype: %s / %s (sum_bases %llu, sum_edges %llu)\n", out.genotype_a.c_str(), out.genotype_b.c_str(),
                    (unsigned long long)out.genotype_sum_bases, (unsigned long long)out.genotype_sum_edges);
        else
            fprintf(stderr, "[vgaligner] genotype: no call\n");
    }
    if (o.genotype_likelihood) {
        if (out.n_likelihood_scored)
            fprintf(stderr, "[vgaligner] genotype-likelihood: %s / %s cost %llu, next +%llu over %llu reads\n", out.likelihood_a.c_str(), out.likelihood_b.c_str(),
                    (unsigned long long)out.likelihood_cost, (unsigned long long)out.likelihood_next, (unsigned long long)out.n_likelihood_scored);
        else
            fprintf(stderr, "[vgaligner] genotype-likelihood: no call\n");
    }
    if (o.path_edit)
        fprintf(stderr, "[vgaligner] path-edit: %llu alignments, %llu paths, %llu too long\n", (unsigned long long)out.n_edit_alignments,
                (unsigned long long)o.paths.n_paths(), (unsigned long long)out.n_edit_too_long);
    if (o.pileup)
        fprintf(stderr, "[vgaligner] Pileup: %llu alignments piled up, %llu leading insertions\n", (unsigned long long)out.n_pileup,
                (unsigned long long)out.n_leading_ins);
    if (o.call_variants)
        fprintf(stderr, "[vgaligner] call-variants: %llu bases tested, %llu calls\n", (unsigned long long)out.n_variant_tested, (unsigned long long)out.n_variant_calls);
    if (o.call_deletions)
        fprintf(stderr, "[vgaligner] call-deletions: %llu runs of %llu alignments, %llu at an end, %llu distinct, %llu calls\n", (unsigned long long)out.n_deletion_runs,
                (unsigned long long)out.n_deletion_alignments, (unsigned long long)out.n_deletion_end_runs, (unsigned long long)out.n_deletion_distinct,
                (unsigned long long)out.n_deletion_calls);
    if (o.call_insertions)
        fprintf(stderr, "[vgaligner] call-insertions: %llu sites, %llu longer than 8\n", (unsigned long long)out.n_insertion_sites, (unsigned long long)out.n_insertion_long);
    if (o.phase)
        fprintf(stderr, "[vgaligner] phase: %llu heterozygous sites, %llu phase sets, %llu reads kept\n", (unsigned long long)out.n_phase_sites,
                (unsigned long long)out.n_phase_sets, (unsigned long long)out.n_phase_reads);
    if (o.phase_join)
        fprintf(stderr, "[vgaligner] phase-join: %llu sets, %llu joins, %llu sets left, %llu agreeing, %llu conflicting links\n", (unsigned long long)out.n_join_sets,
                (unsigned long long)out.n_joins, (unsigned long long)(out.n_join_sets - out.n_joins), (unsigned long long)out.n_join_agree,
                (unsigned long long)out.n_join_conflict);
    if (o.haplotype_paths) {
        fprintf(stderr, "[vgaligner] haplotype-paths: %llu sets, %llu groups with reads, %llu of %llu kept reads scored\n", (unsigned long long)out.n_hap_path_sets,
                (unsigned long long)out.n_hap_path_groups, (unsigned long long)out.n_hap_path_scored, (unsigned long long)out.n_hap_path_kept);
        fprintf(stderr, "[vgaligner] haplotype-paths: %s\n", out.n_hap_path_groups ? out.hap_path_call.c_str() : "no call");
    }
    if (o.path_abundance) {
        if (out.n_abundance_scored) {
            std::string s;
            for (size_t i = 0; i < out.abundance_ppm.size(); i++) s += (i ? ", " : ": ") + std::to_string(out.abundance_ppm[i]) + " ppm";
            fprintf(stderr, "[vgaligner] path-abundance: %llu reads scored of %llu kept, %llu iterations (%s), %zu paths at or above %llu ppm%s\n",
                    (unsigned long long)out.n_abundance_scored, (unsigned long long)out.n_abundance_kept, (unsigned long long)out.abundance_iterations,
                    out.abundance_converged ? "converged" : "not converged", out.abundance_ppm.size(), (unsigned long long)o.abundance_min, s.c_str());
        } else
            fprintf(stderr, "[vgaligner] path-abundance: no call\n");
    }
    if (o.haplotag)
        fprintf(stderr, "[vgaligner] haplotag: %llu rows of %llu reads: %llu a, %llu b, %llu undecided\n", (unsigned long long)out.n_haplotag_rows,
                (unsigned long long)out.n_phase_reads, (unsigned long long)out.n_haplotag_a, (unsigned long long)out.n_haplotag_b,
                (unsigned long long)out.n_haplotag_tied);
    if (o.haplotype_calls)
        fprintf(stderr, "[vgaligner] haplotype-calls: %llu jobs, %llu rows, %llu differ\n", (unsigned long long)out.n_hapcall_jobs,
                (unsigned long long)out.n_hapcall_rows, (unsigned long long)out.n_hapcall_differ);
    if (o.write_console) fputs(o.also_align ? out.alignments_gaf.c_str() : out.chains_gaf.c_str(), stdout);
    trace_mark("done");
    if (getenv("VGA_TRACE"))  // (what the exit has to give back: resident host memory)
        if (FILE *f = fopen("/proc/self/status", "r")) {
            char ln[256];
            while (fgets(ln, sizeof ln, f))
                if (!strncmp(ln, "VmRSS", 5) || !strncmp(ln, "VmHWM", 5) || !strncmp(ln, "RssAnon", 7) || !strncmp(ln, "RssShmem", 8) || !strncmp(ln, "RssFile", 7))
                    fprintf(stderr, "[vgh-trace] %s", ln);
            fclose(f);
        }
    if (o.leave_contexts) {  // the GAF files are closed; what is left is HBM the driver reclaims by itself
        fflush(stdout);
        fflush(stderr);
        _exit(0);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    // This process only maps reads, and its big blocks (anchor arrays, GAF text: 0.1-1.8 GB each, one set per chunk) come and go on
    // worker threads.  glibc gives every thread an arena of 64 MB heaps, so such blocks are mmap'ed and munmap'ed whatever
    // M_MMAP_THRESHOLD says: 1.8 GB of page faults per array set, and a munmap that holds the address-space lock for 0.1-0.2 s
    // while every other thread's page faults and mmaps wait (the DP launches of the next sub-batch among them).  One arena (the
    // brk heap), nothing mmap'ed below 2 GB, nothing trimmed: blocks are recycled from chunk to chunk.  Config 5, 100 000 reads end
    // to end: 6.4 -> 4.3 s (vga_map_batch of a 25 000-read chunk 316 -> 115 ms).  Before the first thread exists.
    if (!getenv("VGA_NO_TUNE_MALLOC")) {
        mallopt(M_ARENA_MAX, 1);
        mallopt(M_MMAP_THRESHOLD, INT32_MAX);
        mallopt(M_TRIM_THRESHOLD, -1);  // (never)
        mallopt(M_TOP_PAD, 256 << 20);
    }
    try {
        if (argc >= 2 && !strcmp(argv[1], "index")) return index_main(argc, argv);
        if (argc >= 2 && !strcmp(argv[1], "map")) return map_main(argc, argv);
        fprintf(stderr, "vgaligner 0.7 (MI355X build)\nUSAGE:\n  vgaligner index -i <graph.gfa> -k <K> [-o prefix] [-e 100] [-m 100] [--device N]\n"
                        "  vgaligner map -i <index> -f <reads.fa|fq> -p abpoa [-o prefix] [-g 1000] [-a 3] [-b 1] [-D -G <graph.gfa>] [-C]\n"
                        "                [--device 0 | --devices 0,1,... | --devices all] [--chunk-reads 32768] [--poa-remain longest|first-edge]\n"
                        "                [--both-strands] [--coverage | --coverage-only] [--path-support] [--pileup]\n"
                        "                [--genotype [--genotype-top 20]]\n"
                        "                [--genotype-likelihood [--genotype-lambda 512] [--genotype-cap 64] [--genotype-top 20]\n"
                        "                                       [--genotype-from support|edit]]\n"
                        "                [--path-edit]\n"
                        "                [--call-variants [--call-error 1280] [--call-min-depth 4] [--call-min-qual 512] [--call-insertions] [--call-deletions]\n"
                        "                                 [--phase [--phase-min-links 2] [--haplotag]]]\n"
                        "                                 (with --haplotag: [--haplotype-calls])\n"
                        "                                 (with --phase: [--phase-join [--phase-join-min-reads 2]])\n"
                        "                                 (with --phase: [--haplotype-paths [--haplotype-paths-cap 64] [--haplotype-paths-top 5]\n"
                        "                                                 [--haplotype-paths-from support|edit]])\n"
                        "                [--path-abundance [--abundance-lambda 512] [--abundance-cap 64] [--abundance-iters 1000] [--abundance-tol 16]\n"
                        "                                  [--abundance-min 10000] [--abundance-from support|edit]]\n");
        return 2;
    } catch (const std::exception &e) {
        fprintf(stderr, "vgaligner: %s\n", e.what());
        return 101;  // a Rust panic exits with 101
    }
}
