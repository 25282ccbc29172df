// cli_main.cpp -- the `metheor` executable: drop-in command line of dohlee/metheor v0.1.9 for the
// measures that run on the MI355X path.  Same subcommands, short/long flags and defaults as the
// reference's clap definitions (src/lib.rs:19-231), same TSV bytes (pdr.rs:95-116, lpmd.rs:137-151),
// same failure behaviour the reference's tests look for (tests/cli_error_handling.rs, tests/*-cli.rs):
// usage errors exit 2 with clap-style text on stderr; run-time failures (the reference panics) exit
// 101 with the panic message on stderr.  There is no CPU fallback: a measure whose device kernel is
// not built yet fails loudly.
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <mutex>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <vector>

#include "../../../include/metheor_hip.h"
#include "../../../include/metheor_host.h"
#include "../mth_regions_host.h"

namespace {

struct Opt {
    const char *long_name;
    char short_name;
    const char *value_name;   // upper-case placeholder
    const char *help;
    const char *def;          // nullptr: no default
    bool required;
    char kind;                // 's' string, 'B' u8, 'U' u32, 'Z' usize, 'I' i32, 'F' a flag: takes no value
};
struct Cmd {
    const char *name;
    const char *about;
    std::vector<Opt> opts;
};

const Opt O_IN = {"input", 'i', "INPUT", "Input BAM file", nullptr, true, 's'};
const Opt O_CPG = {"cpg-set", 'c', "CPG_SET", "(Optional) Specify a predefined set of CpGs (in BED file) to be analyzed", nullptr, false, 's'};
// not in the reference (outer row): one run split over the GPUs of the node by genomic region
const Opt O_GPUS = {"gpus", 'G', "GPUS", "(MI355X extension) Number of GPUs to split the run over, by genomic region", "1", false, 'U'};
// not in the reference either: the .bai files its fixtures ship finally get a reader
const Opt O_REGION = {"region", 'r', "REGION", "(MI355X extension) Only this region: chr or chr:beg-end (1-based, inclusive); needs the BAM index", nullptr, false, 's'};
// not in the reference: the two commands `tag`, then the measure, as one
const Opt O_GENOME = {"genome", 'g', "GENOME", "(MI355X extension) Reference FASTA: derive the methylation calls from it instead of XM:Z tags, as `metheor tag` would; XM:Z tags in the input are ignored", nullptr, false, 's'};
// not in the reference: 5mC calls as current instruments write them, the SAM base-modification tags
const Opt O_MMTAGS = {"mm-tags", 0, "", "(MI355X extension) Take the methylation calls from the MM:Z / ML:B:C base-modification tags (5mC, C+m, in read CpG context) instead of XM:Z tags; XM:Z tags in the input are ignored", nullptr, false, 'F'};
const Opt O_MMTHR = {"mm-threshold", 0, "MM_THRESHOLD", "(MI355X extension) With the MM / ML tags as the source of calls: a listed C whose ML probability is at least this (0..=255) is methylated", "128", false, 'B'};
// not in the reference: LPMD per interval of a BED file, reduced on the device from the pairs table
const Opt O_INTERVALS = {"intervals", 0, "INTERVALS", "(MI355X extension) BED file of intervals: LPMD of each one, as `-c` with all of the interval's positions would give it", nullptr, false, 's'};
// ... and MHL per interval, counted on the device from the reads; on `all` the BED is shared by the two tables
const Opt O_INTERVALS_MHL = {"intervals", 0, "INTERVALS", "BED file of intervals: MHL of each one, from the reads' calls inside it, as `-c` with all of the interval's positions would keep them", nullptr, true, 's'};
const Opt O_INTERVALS_ALL = {"intervals", 0, "INTERVALS", "(MI355X extension) BED file of intervals for --lpmd-intervals, --mhl-intervals, --pdr-intervals, --me-intervals and / or --pm-intervals: each measure restricted to an interval's positions, as `-c` with all of them would", nullptr, false, 's'};
// ... and PDR per interval, counted on the device from the reads
const Opt O_INTERVALS_PDR = {"intervals", 0, "INTERVALS", "BED file of intervals: PDR of each one, from the reads' calls inside it, as `-c` with all of the interval's positions would keep them", nullptr, true, 's'};
// ... and ME / PM per interval, from sixteen counters per interval counted on the device
const Opt O_INTERVALS_QR = {"intervals", 0, "INTERVALS", "BED file of intervals: the value of each one, from the windows of four consecutive calls of every read inside it, as `-c` with all of the interval's positions would keep them", nullptr, true, 's'};
const Opt O_BAI = {"bai", 'b', "BAI", "(MI355X extension) BAM index for --region [default: <input>.bai]", nullptr, false, 's'};

// lib.rs:24-231
const std::vector<Cmd> &commands() {
    static const std::vector<Cmd> c = {
        {"pdr", "Compute proportion of discordant reads (PDR)",
         {O_IN, {"output", 'o', "OUTPUT", "Path to output table file summarizing the result of PDR calculation", nullptr, true, 's'},
          {"min-depth", 'd', "MIN_DEPTH", "Minimum depth of CpG stretches to consider", "10", false, 'U'},
          {"min-cpgs", 'p', "MIN_CPGS", "Minimum number of consecutive CpGs in a CpG stretch to consider", "4", false, 'Z'},
          {"min-qual", 'q', "MIN_QUAL", "Minimum quality for a read to be considered", "10", false, 'B'}, O_CPG, O_GPUS, O_REGION, O_BAI, O_GENOME, O_MMTAGS, O_MMTHR}},
        {"pm", "Compute epipolymorphism",
         {O_IN, {"output", 'o', "OUTPUT", "Path to output table file summarizing the result of PM calculation", nullptr, true, 's'},
          {"min-depth", 'd', "MIN_DEPTH", "Minimum depth of CpG quartets to consider", "10", false, 'U'},
          {"min-qual", 'q', "MIN_QUAL", "Minimum quality for a read to be considered", "10", false, 'B'}, O_CPG, O_GPUS, O_REGION, O_BAI, O_GENOME, O_MMTAGS, O_MMTHR}},
        {"me", "Compute methylation entropy",
         {O_IN, {"output", 'o', "OUTPUT", "Path to output table file summarizing the result of PDR calculation", nullptr, true, 's'},
          {"min-depth", 'd', "MIN_DEPTH", "Minimum depth of CpG quartets to consider", "10", false, 'U'},
          {"min-qual", 'q', "MIN_QUAL", "Minimum quality for a read to be considered", "10", false, 'B'}, O_CPG, O_GPUS, O_REGION, O_BAI, O_GENOME, O_MMTAGS, O_MMTHR}},
        {"fdrp", "Compute fraction of discordant read pairs (FDRP)",
         {{"input", 'i', "INPUT", "Path to input BAM file", nullptr, true, 's'},
          {"output", 'o', "OUTPUT", "Path to output table file summarizing the result of FDRP calculation", nullptr, true, 's'},
          {"min-qual", 'q', "MIN_QUAL", "Minimum quality for a read to be considered", "10", false, 'B'},
          {"min-depth", 'd', "MIN_DEPTH", "Minimum number of reads mapped to a CpG in order to be considered", "10", false, 'Z'},
          {"max-depth", 'D', "MAX_DEPTH", "Maximum number of reads to consider", "40", false, 'Z'},
          {"min-overlap", 'l', "MIN_OVERLAP", "Minimum overlap between two reads to consider in bp", "35", false, 'I'}, O_CPG, O_GPUS, O_REGION, O_BAI, O_GENOME, O_MMTAGS, O_MMTHR}},
        {"qfdrp", "Compute quantitative fraction of discordant read pairs (qFDRP)",
         {{"input", 'i', "INPUT", "Path to input BAM file", nullptr, true, 's'},
          {"output", 'o', "OUTPUT", "Path to output table file summarizing the result of FDRP calculation", nullptr, true, 's'},
          {"min-qual", 'q', "MIN_QUAL", "Minimum quality for a read to be considered", "10", false, 'B'},
          {"min-depth", 'd', "MIN_DEPTH", "Minimum number of reads mapped to a CpG in order to be considered", "10", false, 'Z'},
          {"max-depth", 'D', "MAX_DEPTH", "Maximum number of reads to consider", "40", false, 'Z'},
          {"min-overlap", 'l', "MIN_OVERLAP", "Minimum overlap between two reads to consider in bp", "35", false, 'I'}, O_CPG, O_GPUS, O_REGION, O_BAI, O_GENOME, O_MMTAGS, O_MMTHR}},
        {"mhl", "Compute methylation haplotype load (MHL)",
         {O_IN, {"output", 'o', "OUTPUT", "Path to output table file summarizing the result of MHL calculation", nullptr, true, 's'},
          {"min-depth", 'd', "MIN_DEPTH", "Minimum depth of CpG stretches to consider", "10", false, 'U'},
          {"min-cpgs", 'p', "MIN_CPGS", "Minimum number of consecutive CpGs in a CpG stretch to consider", "4", false, 'Z'},
          {"min-qual", 'q', "MIN_QUAL", "Minimum quality for a read to be considered", "10", false, 'B'}, O_CPG, O_GPUS, O_REGION, O_BAI, O_GENOME, O_MMTAGS, O_MMTHR}},
        {"lpmd", "Compute local pairwise methylation discordance (LPMD)",
         {{"input", 'i', "INPUT", "Path to input BAM file", nullptr, true, 's'},
          {"output", 'o', "OUTPUT", "Path to output table file summarizing the result of LPMD calculation", nullptr, true, 's'},
          {"pairs", 'p', "PAIRS", "(Optional) Concordance information for all CpG pairs", nullptr, false, 's'},
          {"min-distance", 'm', "MIN_DISTANCE", "Minimum distance between CpG pairs to consider", "2", false, 'I'},
          {"max-distance", 'M', "MAX_DISTANCE", "Maximum distance between CpG pairs to consider", "16", false, 'I'},
          {"min-qual", 'q', "MIN_QUAL", "Minimum quality for a read to be considered", "10", false, 'B'}, O_CPG, O_GPUS, O_REGION, O_BAI, O_GENOME, O_MMTAGS, O_MMTHR,
          O_INTERVALS, {"intervals-output", 0, "INTERVALS_OUTPUT", "(MI355X extension) Output table of the per-interval LPMD (needs --intervals)", nullptr, false, 's'}}},
        // not in the reference: any subset of the seven measures from ONE decode of the input (the parameters are shared by every
        // measure that has them, under the single commands' names and defaults; --lpmd-pairs is lpmd's --pairs, whose -p is min-cpgs here)
        {"all", "(MI355X extension) Compute any of the seven measures from one decode of the input",
         {O_IN,
          {"pdr", 0, "PDR", "Output table of PDR", nullptr, false, 's'},
          {"lpmd", 0, "LPMD", "Output table of LPMD", nullptr, false, 's'},
          {"lpmd-pairs", 0, "LPMD_PAIRS", "(Optional) Concordance information for all CpG pairs (needs --lpmd)", nullptr, false, 's'},
          {"mhl", 0, "MHL", "Output table of MHL", nullptr, false, 's'},
          {"me", 0, "ME", "Output table of methylation entropy", nullptr, false, 's'},
          {"pm", 0, "PM", "Output table of epipolymorphism", nullptr, false, 's'},
          {"fdrp", 0, "FDRP", "Output table of FDRP", nullptr, false, 's'},
          {"qfdrp", 0, "QFDRP", "Output table of qFDRP", nullptr, false, 's'},
          {"min-depth", 'd', "MIN_DEPTH", "Minimum depth of CpG stretches / quartets / reads mapped to a CpG to consider", "10", false, 'U'},
          {"min-cpgs", 'p', "MIN_CPGS", "Minimum number of consecutive CpGs in a CpG stretch to consider", "4", false, 'Z'},
          {"min-qual", 'q', "MIN_QUAL", "Minimum quality for a read to be considered", "10", false, 'B'},
          {"min-distance", 'm', "MIN_DISTANCE", "Minimum distance between CpG pairs to consider", "2", false, 'I'},
          {"max-distance", 'M', "MAX_DISTANCE", "Maximum distance between CpG pairs to consider", "16", false, 'I'},
          {"max-depth", 'D', "MAX_DEPTH", "Maximum number of reads to consider", "40", false, 'Z'},
          {"min-overlap", 'l', "MIN_OVERLAP", "Minimum overlap between two reads to consider in bp", "35", false, 'I'},
          O_CPG, O_REGION, O_BAI, O_GENOME, O_MMTAGS, O_MMTHR,
          O_INTERVALS_ALL, {"lpmd-intervals", 0, "LPMD_INTERVALS", "(MI355X extension) Output table of the per-interval LPMD (needs --lpmd and the BED)", nullptr, false, 's'},
          {"mhl-intervals", 0, "MHL_INTERVALS", "(MI355X extension) Output table of the per-interval MHL, one row per line of the BED (needs the BED; an output of its own, --mhl is not needed)", nullptr, false, 's'},
          {"pdr-intervals", 0, "PDR_INTERVALS", "(MI355X extension) Output table of the per-interval PDR, one row per line of the BED (needs the BED; an output of its own, --pdr is not needed)", nullptr, false, 's'},
          {"me-intervals", 0, "ME_INTERVALS", "(MI355X extension) Output table of the per-interval methylation entropy, one row per line of the BED (needs the BED; an output of its own, --me is not needed)", nullptr, false, 's'},
          {"pm-intervals", 0, "PM_INTERVALS", "(MI355X extension) Output table of the per-interval epipolymorphism, one row per line of the BED (needs the BED; an output of its own, --pm is not needed)", nullptr, false, 's'}}},
        // not in the reference: MHL of a region, as Guo et al. (2017) define it, for every interval of a BED file
        {"mhl-regions", "(MI355X extension) Compute methylation haplotype load (MHL) per interval of a BED file",
         {O_IN, {"output", 'o', "OUTPUT", "Path to output table: chrom, start, end, name, mhl, n_reads, max_cpgs, one row per line of the BED", nullptr, true, 's'},
          O_INTERVALS_MHL,
          {"min-depth", 'd', "MIN_DEPTH", "Minimum number of contributing reads of an interval (fewer: NaN)", "10", false, 'U'},
          {"min-cpgs", 'p', "MIN_CPGS", "Minimum number of CpGs of a read inside an interval for the read to contribute", "4", false, 'Z'},
          {"min-qual", 'q', "MIN_QUAL", "Minimum quality for a read to be considered", "10", false, 'B'}, O_CPG, O_GPUS, O_GENOME, O_MMTAGS, O_MMTHR}},
        // not in the reference: PDR of a region (Landau et al. 2014) for every interval of a BED file
        {"pdr-regions", "(MI355X extension) Compute proportion of discordant reads (PDR) per interval of a BED file",
         {O_IN, {"output", 'o', "OUTPUT", "Path to output table: chrom, start, end, name, pdr, n_concordant, n_discordant, n_methylated, one row per line of the BED", nullptr, true, 's'},
          O_INTERVALS_PDR,
          {"min-depth", 'd', "MIN_DEPTH", "Minimum number of contributing reads of an interval (fewer: NaN)", "10", false, 'U'},
          {"min-cpgs", 'p', "MIN_CPGS", "Minimum number of CpGs of a read inside an interval for the read to contribute", "4", false, 'Z'},
          {"min-qual", 'q', "MIN_QUAL", "Minimum quality for a read to be considered", "10", false, 'B'}, O_CPG, O_GPUS, O_GENOME, O_MMTAGS, O_MMTHR}},
        // not in the reference: ME (Xie et al. 2011) and PM (Landan et al. 2012) of a region, every window of four consecutive calls inside
        // an interval pooled into one histogram, for every interval of a BED file
        {"me-regions", "(MI355X extension) Compute methylation entropy per interval of a BED file",
         {O_IN, {"output", 'o', "OUTPUT", "Path to output table: chrom, start, end, name, me, n_patterns, n_reads, one row per line of the BED", nullptr, true, 's'},
          O_INTERVALS_QR,
          {"min-depth", 'd', "MIN_DEPTH", "Minimum number of patterns (windows of four CpGs) of an interval (fewer: NaN)", "10", false, 'U'},
          {"min-qual", 'q', "MIN_QUAL", "Minimum quality for a read to be considered", "10", false, 'B'}, O_CPG, O_GPUS, O_GENOME, O_MMTAGS, O_MMTHR}},
        {"pm-regions", "(MI355X extension) Compute epipolymorphism per interval of a BED file",
         {O_IN, {"output", 'o', "OUTPUT", "Path to output table: chrom, start, end, name, pm, n_patterns, n_reads, one row per line of the BED", nullptr, true, 's'},
          O_INTERVALS_QR,
          {"min-depth", 'd', "MIN_DEPTH", "Minimum number of patterns (windows of four CpGs) of an interval (fewer: NaN)", "10", false, 'U'},
          {"min-qual", 'q', "MIN_QUAL", "Minimum quality for a read to be considered", "10", false, 'B'}, O_CPG, O_GPUS, O_GENOME, O_MMTAGS, O_MMTHR}},
        {"tag", "Add bismark XM tag to BAM file",
         {{"input", 'i', "INPUT", "", nullptr, true, 's'}, {"output", 'o', "OUTPUT", "", nullptr, true, 's'},
          {"genome", 'g', "GENOME", "", nullptr, true, 's'},
          // not in the reference (its writer is bam::Format::Sam, tag.rs:406): the tagged records as a BGZF-compressed BAM made on the device
          {"output-format", 'O', "OUTPUT_FORMAT", "(MI355X extension) Format of the output alignment file: sam or bam", "sam", false, 's'},
          // not in the reference either: the .bai of that BAM, built on the device beside the records (mth_bai.hip), as <OUTPUT>.bai
          {"write-index", 0, "", "(MI355X extension) with -O bam, also write the BAM index <OUTPUT>.bai, built on the device", nullptr, false, 'F'}}},
    };
    return c;
}

void print_main_help(FILE *f) {
    fprintf(f, "Summarizes the heterogeneity of DNA methylation states using BAM files.\n\nUsage: metheor <COMMAND>\n\nCommands:\n");
    for (const Cmd &c : commands()) fprintf(f, "  %-11s %s\n", c.name, c.about);
    fprintf(f, "  help        Print this message or the help of the given subcommand(s)\n\nOptions:\n"
               "  -h, --help     Print help\n  -V, --version  Print version\n");
}

std::string usage_line(const Cmd &c) {
    std::string u = std::string("Usage: metheor ") + c.name + " [OPTIONS]";
    for (const Opt &o : c.opts) if (o.required) u += std::string(" --") + o.long_name + " <" + o.value_name + ">";
    return u;
}

void print_cmd_help(FILE *f, const Cmd &c) {
    fprintf(f, "%s\n\n%s\n\nOptions:\n", c.about, usage_line(c).c_str());
    const Opt *ext = nullptr, *ext_flag = nullptr;
    for (const Opt &o : c.opts) {
        // `tag --help` on stdout is the reference's text to the byte (tests/test_genome_cli_args.py pins it): tag's extensions are
        // listed on stderr instead, after the help
        if (!strcmp(c.name, "tag") && !strcmp(o.long_name, "output-format")) { ext = &o; continue; }
        if (!strcmp(c.name, "tag") && !strcmp(o.long_name, "write-index")) { ext_flag = &o; continue; }
        std::string left = o.short_name ? std::string("  -") + o.short_name + ", --" + o.long_name + " <" + o.value_name + ">"
                                        : std::string("      --") + o.long_name + " <" + o.value_name + ">";      // (a long-only option)
        if (o.kind == 'F') left = std::string("      --") + o.long_name;                                             // (a flag)
        fprintf(f, "%-34s %s%s%s%s\n", left.c_str(), o.help, o.def ? " [default: " : "", o.def ? o.def : "", o.def ? "]" : "");
    }
    fprintf(f, "  -h, --help                       Print help\n");
    if (ext) { fflush(f); fprintf(stderr, "\nExtension:\n  -O, --output-format <OUTPUT_FORMAT> %s [default: %s]\n", ext->help, ext->def); }
    if (ext_flag) fprintf(stderr, "      --%-30s %s\n", ext_flag->long_name, ext_flag->help);
}

[[noreturn]] void usage_error(const Cmd *c, const std::string &msg) {
    fprintf(stderr, "error: %s\n\n%s\n\nFor more information, try '--help'.\n", msg.c_str(),
            c ? usage_line(*c).c_str() : "Usage: metheor <COMMAND>");
    exit(2);
}

// the reference panics on run-time failures: message on stderr, exit status 101
// (with --gpus N the failing shard's thread ends the process: _exit, the other shards' threads are mid-run)
std::atomic<bool> g_threads{false};
[[noreturn]] void die(const std::string &msg) {
    fprintf(stderr, "%s\n", msg.c_str());
    if (g_threads.load()) { fflush(nullptr); _exit(101); }
    exit(101);
}

bool parse_number(const Opt &o, const std::string &v, int64_t &out, std::string &why) {
    if (v.empty()) { why = "cannot parse integer from empty string"; return false; }
    char *end = nullptr;
    errno = 0;
    const long long x = strtoll(v.c_str(), &end, 10);
    if (*end != 0 || errno) { why = "invalid digit found in string"; return false; }
    int64_t lo = 0, hi = 0;
    switch (o.kind) {
        case 'B': lo = 0; hi = 255; break;
        case 'U': lo = 0; hi = 4294967295LL; break;
        case 'Z': lo = 0; hi = INT64_MAX; break;
        case 'I': lo = INT32_MIN; hi = INT32_MAX; break;
        default: break;
    }
    if (x < lo || x > hi) {
        why = o.kind == 'B' ? v + " is not in 0..=255"
            : (x < 0 && o.kind != 'I') ? "invalid digit found in string" : "number too large to fit in target type";
        return false;
    }
    out = x;
    return true;
}

struct Args {
    std::map<std::string, std::string> s;
    std::map<std::string, int64_t> n;
    bool has(const char *k) const { return s.count(k) != 0; }
};

Args parse_args(const Cmd &c, int argc, char **argv, int first) {
    Args a;
    if (first >= argc) { print_cmd_help(stderr, c); exit(2); }   // arg_required_else_help
    for (int i = first; i < argc; ++i) {
        std::string tok = argv[i];
        if (tok == "-h" || tok == "--help") { print_cmd_help(stdout, c); exit(0); }
        const Opt *o = nullptr;
        std::string val;
        bool have_val = false;
        if (tok.rfind("--", 0) == 0) {
            const size_t eq = tok.find('=');
            const std::string name = tok.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
            for (const Opt &x : c.opts) if (name == x.long_name) o = &x;
            if (eq != std::string::npos) { val = tok.substr(eq + 1); have_val = true; }
        } else if (tok.size() >= 2 && tok[0] == '-') {
            for (const Opt &x : c.opts) if (tok[1] == x.short_name) o = &x;
            if (o && tok.size() > 2) { val = tok.substr(tok[2] == '=' ? 3 : 2); have_val = true; }
        }
        if (!o) usage_error(&c, "unexpected argument '" + tok + "' found");
        if (o->kind == 'F') {
            if (have_val) usage_error(&c, "unexpected value '" + val + "' for '--" + o->long_name + "' found; no more were expected");
            a.s[o->long_name] = "true";
            continue;
        }
        if (!have_val) {
            if (i + 1 >= argc) usage_error(&c, std::string("a value is required for '--") + o->long_name + " <" + o->value_name + ">' but none was supplied");
            val = argv[++i];
            // clap (no allow_hyphen_values / allow_negative_numbers in lib.rs): a separate token that
            // looks like a flag is never taken as a value ("-5" after --min-depth); --opt=-5 is
            if (val.size() > 1 && val[0] == '-')
                usage_error(&c, "unexpected argument '" + val + "' found");
        }
        if (o->kind == 's') a.s[o->long_name] = val;
        else {
            int64_t x;
            std::string why;
            if (!parse_number(*o, val, x, why))
                usage_error(&c, "invalid value '" + val + "' for '--" + o->long_name + " <" + o->value_name + ">': " + why);
            a.n[o->long_name] = x;
            a.s[o->long_name] = val;
        }
    }
    std::string missing;
    for (const Opt &o : c.opts) {
        if (o.required && !a.has(o.long_name)) missing += std::string("\n  --") + o.long_name + " <" + o.value_name + ">";
        if (o.def && !a.has(o.long_name)) { a.n[o.long_name] = strtoll(o.def, nullptr, 10); }
    }
    if (!missing.empty()) usage_error(&c, "the following required arguments were not provided:" + missing);
    return a;
}

// ---- decoded input as per-contig batches --------------------------------------------------------
// A contig's reads are a contiguous slice of the decoded SoA (the file is coordinate-sorted), so the
// batch points straight into the decoder's arrays; only the CSR offsets are rebased (4 B/read).  A
// contig that contains a read without any aligned base (start = -1) is copied without those reads.
// --gpus N: the run is N shards, one host thread and one device context each (shard r on device r mod the devices
// present, or mod METHEOR_DEVICES).  Every shard loads its own run of BGZF blocks (mth_host_plan_shard: no index, no
// router), owns a (tid, pos) interval and formats its rows into memory; the parts concatenated in shard order are the
// unsharded file.  The only exchange is the RCCL all-reduce of the four LPMD counters (mth_allreduce_lpmd).
// METHEOR_SHARD_HALO: bp of reads loaded before the interval (default 65536; must cover the longest alignment + FDRP's
// 201-bp window, checked).
struct Shard {
    int rank = 0, world = 1, device = 0;
    int64_t halo = 65536;
    mth_host_shard_t plan;
    int xm_min_mapq = 0;
    // --region chr[:beg-end]: the plan comes from the .bai (mth_host_plan_region) instead of a byte-range cut
    bool region = false;
    std::string region_name, bai;
    int32_t r_beg = 0, r_end = INT32_MAX;          // 0-based [r_beg, r_end); INT32_MAX = to the end of the contig's data
    bool order_free = false;                       // set by lpmd / me / pm: their result does not depend on the record order (see load())
    bool planned() const { return world > 1 || region; }
};
thread_local Shard g_shard;

// what one shard contributes to the output files (filled through open_memstream when world > 1)
struct Part { char *out = nullptr; size_t out_len = 0; char *pairs = nullptr; size_t pairs_len = 0; std::vector<int64_t> iv_c, iv_d;
              std::vector<uint32_t> mr_iv, mr_len; std::vector<uint64_t> mr_runs, mr_reads;
              std::vector<uint64_t> pr_m, pr_u, pr_d;
              std::vector<uint64_t> qr_bins, qr_reads; };
thread_local Part *g_part = nullptr;

// the shards' threads meet here once: the last to arrive runs the collective for all of them
struct Gang {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<mth_ctx_t *> ctxs;
    int arrived = 0, rc = MTH_OK;
    bool done = false;
} g_gang;

struct Contig {
    int32_t tid;
    int32_t region_beg = 0, region_end = -1;   // owned positions (-1: to the contig's end); a shard may own part of a contig
    const int32_t *start, *end;
    const uint8_t *mapq;
    const uint32_t *pos;
    const uint16_t *rel;
    size_t n_reads, n_cpgs;
    std::vector<uint32_t> off;
    int32_t max_span = 0, max_end = -1;
    uint64_t r0 = 0, r1 = 0;   // device-decoded input: the contig's reads in the decoded stream
    // owned copies (only when filtering was needed)
    std::vector<int32_t> o_start, o_end;
    std::vector<uint8_t> o_mapq;
    std::vector<uint32_t> o_pos;
    std::vector<uint16_t> o_rel;
    // host-decoded input: the contig holds a call at position -1 and was shifted up by MTH_GROUP_MINUS_ONE_BASE (the o_ copies); it goes
    // in as a contig group of one, defined by load() on the context the batches go to
    bool lifted = false;
    int32_t group = 0;
};

struct Input {
    mth_host_t *h = nullptr;
    std::vector<Contig> contigs;
    // the reads re-ordered by (tid, start) -- order-free measures on an input that is not coordinate-sorted (sort_reads)
    std::vector<int32_t> s_tid, s_start, s_end;
    std::vector<uint8_t> s_mapq;
    std::vector<uint64_t> s_off;
    std::vector<uint32_t> s_pos;
    std::vector<uint16_t> s_rel;
    mth_ctx_t *ctx = nullptr;   // set when the records were decoded on the device (the batches live in its HBM)
    bool device = false;
    bool file_order = false;               // pdr / mhl / fdrp / qfdrp on input that is not coordinate-sorted: no batches, the decoded stream itself (mth_fileorder_run)
    uint32_t dec_flags = 0;                // mth_decoded_contigs' flags of the decoded stream (file_order: whether mth_decoded_sort may take it)
    std::vector<uint8_t> unbatched_mapq;   // mapq of the records that entered no batch (no contig / no aligned base): lpmd.rs:176-179 counts them
};

// METHEOR_TIMING=1: phase wall times on stderr (never stdout)
struct Phase {
    const char *name;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit Phase(const char *n) : name(n) {}
    ~Phase() {
        if (!getenv("METHEOR_TIMING")) return;
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[metheor timing] %-28s %.3f s\n", name, s);
    }
};

// End of a run, output files closed.  Releasing gigabytes of device buffers, unmapping the input and unloading the HIP
// runtime cost tens of milliseconds that nobody reads the result of: the process leaves through _exit and the driver
// reclaims everything (METHEOR_TEARDOWN=1 keeps the orderly release, e.g. under a leak checker).
int finish(mth_ctx_t *ctx, mth_host_t *h) {
    {   // a CIGAR P operation was decoded: this engine takes it as "no query base, no reference base" (the SAM specification's meaning);
        // what the reference's BAM crate does with it cannot be checked here -- the note says what THIS engine did
        static std::atomic<bool> said{false};
        if ((((ctx ? mth_notes(ctx) : 0u) | mth_host_notes()) & MTH_NOTE_CIGAR_PAD) && !said.exchange(true))
            fprintf(stderr, "metheor: note: the input holds CIGAR 'P' (padding) operations; they were taken as covering no query base and no "
                            "reference base\n");
    }
    {   // --mm-tags: records whose MM / ML cannot be placed on SEQ gave no call
        static std::atomic<bool> said{false};
        if (ctx && (mth_notes(ctx) & MTH_NOTE_MODTAG_SKIPPED) && !said.exchange(true))
            fprintf(stderr, "metheor: note: --mm-tags: the input holds records without SEQ, with hard clips or with an MN field that differs from "
                            "the length of SEQ; they contributed no methylation call\n");
    }
    if (g_shard.world > 1) return 0;      // a shard's thread: main() writes the files and leaves
    if (getenv("METHEOR_TEARDOWN")) {
        Phase ph("teardown");
        { Phase p1("  device context destroy"); mth_ctx_destroy(ctx); }
        { Phase p2("  input close (munmap)"); mth_host_close(h); }
        return 0;
    }
    fflush(nullptr);
    _exit(0);
}

void check(mth_ctx_t *ctx, int rc) {
    if (rc == MTH_OK) return;
    std::string m = std::string("metheor (MI355X path): ") + mth_strerror(rc);
    if (ctx && mth_last_error(ctx)[0]) m += std::string(" -- ") + mth_last_error(ctx);
    die(m);
}

// HIP initialisation takes 70-140 ms: on the device load path it runs on its own thread while the main thread opens the
// file, parses --cpg-set and builds the BGZF block table.  Errors are reported by whoever joins (file errors first).
struct CtxFuture {
    std::thread th;
    mth_ctx_t *ctx = nullptr;
    int rc = MTH_OK;
    void start() {
        const int device = g_shard.device;
        th = std::thread([this, device] {
            Phase ph("device context (overlapped)");
            rc = mth_ctx_create(device, &ctx);
        });
    }
    void wait() { if (th.joinable()) th.join(); }
    mth_ctx_t *get() {
        wait();
        if (rc != MTH_OK) die(std::string("metheor (MI355X path): ") + mth_strerror(rc));
        return ctx;
    }
};

mth_ctx_t *make_ctx() {
    Phase ph("device context");
    mth_ctx_t *ctx = nullptr;
    const int rc = mth_ctx_create(g_shard.device, &ctx);
    if (rc != MTH_OK) die(std::string("metheor (MI355X path): ") + mth_strerror(rc));
    return ctx;
}

// ---- the reference genome (`tag`, and --genome on the measures) -------------------------------------------------------------------
// tag.rs:412-431: open the FASTA, fetch every @SQ contig of the input's header up to its LN.  One host copy per process (--gpus N:
// read once by main(), uploaded by every shard's context).
struct Genome {
    std::string path;                      // empty: no --genome
    bool loaded = false;
    std::vector<std::vector<uint8_t>> seqs;
    std::vector<const uint8_t *> ptr;
    std::vector<int64_t> ln, got;
    // the device route (mth_tag_set_genome_fasta): a bgzip-compressed FASTA, or a plain one under METHEOR_GENOME_DEVICE=1.  The
    // FASTA stays open: every context packs its genome from the one mapping, by the one set of layout rows
    bool device = false;
    mth_fasta_t *fa = nullptr;
    mth_host_fasta_map_t map{};
    std::vector<mth_fasta_row_t> rows;
};
Genome g_genome;

// the messages and the status are `tag`'s (tag.rs:414-417, 427); on_fail runs before the process ends (tag flushes its output)
template <class F>
mth_fasta_t *genome_open(const std::string &path, F on_fail) {
    mth_fasta_t *fa = nullptr;
    char err[1024];
    if (mth_host_fasta_open(path.c_str(), &fa, err, sizeof err) != 0) { on_fail(); die(std::string("Error opening reference genome file: ") + err); }
    return fa;
}
template <class F>
void genome_fetch(mth_fasta_t *fa, mth_host_t *h, Genome &g, F on_fail) {
    const int n_refs = mth_host_n_refs(h);
    g.seqs.assign((size_t)n_refs, {}); g.ptr.assign((size_t)n_refs, nullptr); g.ln.assign((size_t)n_refs, 0); g.got.assign((size_t)n_refs, 0);
    for (int t = 0; t < n_refs; ++t) {
        const uint8_t *p = nullptr;
        int64_t n = 0;
        g.ln[(size_t)t] = mth_host_ref_len(h, t);
        if (mth_host_fasta_fetch(fa, mth_host_ref_name(h, t), g.ln[(size_t)t], &p, &n) != 0) { on_fail(); die("Error fetching reference genome sequence.: " + std::string(mth_host_fasta_last_error(fa))); }
        g.seqs[(size_t)t].assign(p, p + n);
        g.ptr[(size_t)t] = g.seqs[(size_t)t].data(); g.got[(size_t)t] = n;
    }
    g.loaded = true;
}
bool genome_wants_device(const mth_fasta_t *fa) {
    const char *e = getenv("METHEOR_GENOME_DEVICE");
    return mth_host_fasta_compressed(fa) || (e && atoi(e) != 0);
}
// the device route's host part: the mapping (populated) and every @SQ contig's layout row, with the fetch's errors and texts
template <class F>
void genome_layout(mth_fasta_t *fa, mth_host_t *h, Genome &g, F on_fail) {
    auto fail = [&] { on_fail(); die("Error fetching reference genome sequence.: " + std::string(mth_host_fasta_last_error(fa))); };
    const int n_refs = mth_host_n_refs(h);
    g.ln.assign((size_t)n_refs, 0); g.rows.assign((size_t)n_refs, mth_fasta_row_t{});
    for (int t = 0; t < n_refs; ++t) {
        mth_host_fasta_row_t r;
        g.ln[(size_t)t] = mth_host_ref_len(h, t);
        if (mth_host_fasta_layout(fa, mth_host_ref_name(h, t), g.ln[(size_t)t], &r) != 0) fail();
        g.rows[(size_t)t] = mth_fasta_row_t{r.src_off, r.n_bases, r.line_bases, r.line_width, r.name};
    }
    if (mth_host_fasta_map(fa, &g.map) != 0) fail();
    g.fa = fa; g.device = true; g.loaded = true;
}
// the genome into a context: the host copy's bases, or the FASTA's bytes packed on the device.  A plain file whose text does not
// have the layout its index states (METHEOR_GENOME_DEVICE=1: the device route verifies every byte) falls back to the host read,
// which gives today's result or today's error; on a compressed file the same finding ends the run.
template <class F>
void genome_upload(mth_ctx_t *ctx, mth_host_t *h, Genome &g, F on_fail) {
    static std::mutex mu;                  // --gpus N: the shards share g
    bool device;
    { std::lock_guard<std::mutex> lk(mu); device = g.device; }
    if (device) {
        const bool timing = getenv("METHEOR_TIMING") != nullptr;
        if (timing) mth_timing_enable(ctx, 1);
        int rc;
        {
            Phase ph("  genome FASTA -> device");
            const mth_fasta_blocks_t blk{g.map.coff, g.map.csize, g.map.isize, g.map.n_blocks};
            rc = mth_tag_set_genome_fasta(ctx, g.map.file, g.map.file_bytes, g.map.compressed ? &blk : nullptr, (int32_t)g.ln.size(), g.ln.data(), g.rows.data());
        }
        if (timing) {
            for (const char *k : {"k_inflate", "k_crc32", "k_fasta_pack"}) {
                double ms = 0;
                uint64_t n = 0;
                if (mth_timing_get(ctx, k, &ms, &n) == MTH_OK && n) fprintf(stderr, "[metheor timing]     genome/%-14s %.3f ms in %llu launches\n", k, ms * (double)n, (unsigned long long)n);
            }
            mth_timing_reset(ctx); mth_timing_enable(ctx, 0);
        }
        if (rc == MTH_OK) return;
        if (rc != MTH_ERR_FORMAT) check(ctx, rc);
        std::lock_guard<std::mutex> lk(mu);
        if (g.map.compressed) { on_fail(); die("Error fetching reference genome sequence.: " + std::string(mth_last_error(ctx))); }
        if (timing) fprintf(stderr, "[metheor timing]   genome FASTA -> device refused (%s): host read instead\n", mth_last_error(ctx));
        if (g.device) { genome_fetch(g.fa, h, g, on_fail); g.device = false; }
    }
    check(ctx, mth_tag_set_genome(ctx, (int32_t)g.ln.size(), g.ln.data(), g.ptr.data(), g.got.data()));
}
// --genome of a measure: read once, before any output file exists
template <class F>
void genome_read_once(mth_host_t *h, F on_fail) {
    if (g_genome.path.empty() || g_genome.loaded) return;
    mth_fasta_t *fa = genome_open(g_genome.path, on_fail);
    if (genome_wants_device(fa)) {
        Phase ph("  genome FASTA map + layout");
        genome_layout(fa, h, g_genome, on_fail);
        return;
    }
    Phase ph("  genome FASTA read");
    genome_fetch(fa, h, g_genome, on_fail);
    mth_host_fasta_close(fa);
}
// --mm-tags: set by main(), put on every context (each --gpus shard's too) by load_on_device
bool g_modtags = false;
uint32_t g_mm_threshold = 128;
const char *const kNoHostModtags =
    "--mm-tags needs the device record decode: the full host decoder (METHEOR_HOST_DECODE=1, or input it has to take: records without a "
    "contig or an aligned base, contigs not grouped) has no MM / ML form";
const char *const kNoHostGenome =
    "--genome needs the device record decode: the full host decoder (METHEOR_HOST_DECODE=1, or input it has to take: records without a "
    "contig or an aligned base, contigs not grouped) has no genome form -- run `metheor tag` first and give the measure its output";

// a failed decode call as the reference's panic
[[noreturn]] void die_decode_format(mth_ctx_t *ctx, const char *what) {
    const std::string m = mth_last_error(ctx);
    if (m.rfind("modtags:", 0) == 0) die(std::string("metheor (MI355X path): ") + mth_strerror(MTH_ERR_FORMAT) + " -- " + m);  // --mm-tags: MM / ML break the rule
    if (m.rfind("tag:", 0) == 0) die(std::string("metheor (MI355X path): ") + mth_strerror(MTH_ERR_FORMAT) + " -- " + m);      // --genome: determine_xm_tag_string panics
    if (m.find("XM") != std::string::npos) die("Error reading XM tag in BAM record. Make sure the reads are aligned using Bismark!");   // readutil.rs:46
    die(std::string("Error reading BAM record. ") + what);
}

// Device-side record decode (mth_decode_records): the host inflates BGZF and walks the record boundaries, every
// window goes to the GPU as raw bytes, and the SoA the measures read is built in HBM -- no record / XM parsing and
// no SoA assembly on host threads (--cpg-set is applied by the decode kernel).  Not used with
// METHEOR_HOST_DECODE=1, or when the file has records the batches cannot hold as they are (no contig, no aligned
// base, contigs not grouped): those fall back to the host decoder below.
struct StreamState { mth_ctx_t *ctx = nullptr; bool first = true; int rc = MTH_OK; };
int window_to_device(void *user, const uint8_t *buf, const uint64_t *rec_off, uint64_t n_rec) {
    StreamState *st = static_cast<StreamState *>(user);
    mth_decoded_t d;
    st->rc = mth_decode_records(st->ctx, buf, rec_off[n_rec], rec_off, n_rec, MTH_MEM_HOST, st->first ? 0 : 1, &d);
    st->first = false;
    return st->rc == MTH_OK ? 0 : 1;
}

// Whole load path on the device (mth_bgzf_decode): the file's bytes go to the GPU as they are, BGZF inflate, record
// boundaries and record decode all happen there.  Needs every BGZF block to hold whole records (what htslib-family
// writers produce).  For a file where that does not hold (htsjdk / Picard, sambamba, ...: blocks cut at a byte count) the
// chunks go through mth_bgzf_decode_straddle instead -- under --region always (nothing else can load a part of such a file),
// for a whole file when METHEOR_DEVICE_STRADDLE=1 (which route is the faster one there: profiles/straddle_walk.md) -- with a
// phase line of its own.  Returns false, with the context reset, when the file is left to the host walk.
// --gpus N by default keeps needing whole records per block: a shard's first block has no verified entry without its neighbour's
// chain.  METHEOR_SHARD_STRADDLE=1 opens it to such files (shard_straddle_load below).
const char *const kStraddlePhase = "  device inflate + straddle walk + decode";

// the chunk loop over blocks [blk_beg, bz.n_blocks) (bz.header_bytes: inflated bytes of the first block before the first record);
// straddle: records may cross blocks and chunks (the library carries the unfinished record from call to call), region_tail: the
// last block may end inside a record that is not wanted.  -> MTH_OK or MTH_ERR_UNALIGNED
int load_chunks(Input &in, const mth_host_bgzf_t &bz, uint64_t blk_beg, bool straddle, bool region_tail) {
    // Chunks of whole blocks.  The first is small (<= 512 MiB of file bytes) so that the GPU starts early; every later chunk
    // (<= 2 GiB; METHEOR_CHUNK_GROWTH makes the sizes grow geometrically instead -- measured slower, profiles/r02_e2e.md) is copied to the device by a helper thread on a side stream (mth_bgzf_stage) while the chunk before it is
    // being inflated and decoded -- only the first copy is exposed.  METHEOR_DEVICE_CHUNK_MB sets both sizes,
    // METHEOR_NO_STAGE=1 copies every chunk in line.
    size_t chunk_first = (size_t)512 << 20, chunk = (size_t)2 << 30, growth = 64;
    if (const char *e = getenv("METHEOR_DEVICE_CHUNK_MB")) { const long k = atol(e); if (k >= 1 && k <= 65536) { chunk_first = chunk = (size_t)k << 20; growth = 1; } }
    if (const char *e = getenv("METHEOR_FIRST_CHUNK_MB")) { const long k = atol(e); if (k >= 1 && k <= 65536) chunk_first = (size_t)k << 20; }
    if (const char *e = getenv("METHEOR_CHUNK_GROWTH")) { const long k = atol(e); if (k >= 1 && k <= 64) growth = (size_t)k; }
    const bool stage = !getenv("METHEOR_NO_STAGE");
    const bool timing = getenv("METHEOR_TIMING") != nullptr;
    struct Chunk { uint64_t b0, b1, base, nbytes, ubytes; };
    std::vector<Chunk> chunks;
    uint64_t total_u = 0;
    for (uint64_t b0 = blk_beg; b0 < bz.n_blocks;) {
        size_t lim = chunk_first;
        for (size_t k = 0; k < chunks.size() && lim < chunk; ++k) lim = std::min(chunk, lim * growth);
        uint64_t b1 = b0, ubytes = 0;
        while (b1 < bz.n_blocks && (b1 == b0 || bz.coff[b1] + bz.csize[b1] - bz.coff[b0] <= lim)) { ubytes += bz.isize[b1]; ++b1; }
        chunks.push_back(Chunk{b0, b1, bz.coff[b0], bz.coff[b1 - 1] + bz.csize[b1 - 1] + 8 - bz.coff[b0], ubytes});   // incl. the last block's CRC32 + ISIZE trailer
        total_u += ubytes;
        b0 = b1;
    }
    if (chunks.empty()) chunks.push_back(Chunk{blk_beg, blk_beg, 0, 0, 0});
    bool first = true;
    uint64_t hdr_left = bz.header_bytes;      // header bytes still ahead of the next chunk's inflated stream
    uint64_t done_u = 0;
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        const Chunk &c = chunks[ci];
        const uint64_t first_byte = std::min<uint64_t>(hdr_left, c.ubytes);
        if (c.b1 > c.b0 && hdr_left > c.ubytes && ci + 1 < chunks.size()) {       // a chunk made of header only
            if (timing) fprintf(stderr, "[metheor load] chunk %zu of %zu: %llu blocks, %llu file bytes, header only, not loaded\n", ci + 1, chunks.size(),
                                (unsigned long long)(c.b1 - c.b0), (unsigned long long)c.nbytes);
            hdr_left -= c.ubytes;
            continue;
        }
        if (stage && ci + 1 < chunks.size() && chunks[ci + 1].nbytes)
            check(in.ctx, mth_bgzf_stage(in.ctx, bz.file + chunks[ci + 1].base, chunks[ci + 1].nbytes));
        std::vector<uint64_t> rel((size_t)(c.b1 - c.b0));
        for (uint64_t k = c.b0; k < c.b1; ++k) rel[(size_t)(k - c.b0)] = bz.coff[k] - c.base;
        mth_decoded_t d;
        int rc;
        mth_load_stats_t ls0{}, ls1{};
        if (timing) check(in.ctx, mth_load_stats(in.ctx, &ls0));
        if (straddle) {
            // the next chunk is staged from its planned file offset all the same: the record a chunk ends in travels in the carry
            const unsigned flags = (first ? 0u : MTH_STRADDLE_APPEND) | (ci + 1 < chunks.size() ? 0u : (region_tail ? MTH_STRADDLE_DROP_TAIL : MTH_STRADDLE_LAST));
            mth_straddle_info_t info;
            rc = mth_bgzf_decode_straddle(in.ctx, bz.file + c.base, c.nbytes, rel.data(), bz.csize + c.b0, bz.isize + c.b0, c.b1 - c.b0, first_byte, flags, &d, &info);
            if (getenv("METHEOR_TIMING"))       // one line per library call: what the walk needed, and what travels into the next chunk
                fprintf(stderr, "[metheor straddle] chunk %zu of %zu: %llu blocks, %u rounds, %u blocks repaired, %llu bytes carried\n", ci + 1, chunks.size(),
                        (unsigned long long)(c.b1 - c.b0), info.rounds, info.repaired_blocks, (unsigned long long)info.carry_bytes);
        } else {
            rc = mth_bgzf_decode(in.ctx, bz.file + c.base, c.nbytes, rel.data(), bz.csize + c.b0, bz.isize + c.b0, c.b1 - c.b0, first_byte, first ? 0 : 1, &d);
        }
        if (timing) {                           // one line per library call, both routes: which way the chunk's file bytes went up
            check(in.ctx, mth_load_stats(in.ctx, &ls1));
            const char *how = ls1.staged_calls > ls0.staged_calls ? "staged" : ls1.pieced_calls > ls0.pieced_calls ? "pieced" : "in line";
            fprintf(stderr, "[metheor load] chunk %zu of %zu: %llu blocks, %llu file bytes, %s, %llu piece launches, %llu records so far\n", ci + 1, chunks.size(), (unsigned long long)(c.b1 - c.b0),
                    (unsigned long long)c.nbytes, how, (unsigned long long)(ls1.pieced_launches - ls0.pieced_launches), (unsigned long long)(rc == MTH_OK ? d.n_reads : 0));
        }
        hdr_left -= first_byte;
        if (rc == MTH_ERR_UNALIGNED) { check(in.ctx, mth_reset(in.ctx)); return rc; }
        if (rc == MTH_ERR_FORMAT) die_decode_format(in.ctx, "corrupt BGZF block or BAM record");
        check(in.ctx, rc);
        done_u += c.ubytes;
        if (first && ci + 1 < chunks.size() && done_u) {
            // size the decoded arrays once from the first chunk's yield (reads and calls per inflated byte, +3 %)
            const double f = 1.03 * (double)total_u / (double)done_u;
            check(in.ctx, mth_decode_reserve(in.ctx, (uint64_t)((double)d.n_reads * f) + 4096, (uint64_t)((double)d.n_cpgs * f) + 4096));
        }
        first = false;
    }
    if (timing) {
        mth_load_stats_t ls{};
        check(in.ctx, mth_load_stats(in.ctx, &ls));
        fprintf(stderr, "[metheor load] %llu reallocations of the decoded arrays, %llu staged copies not taken\n", (unsigned long long)ls.decode_reallocs, (unsigned long long)ls.stage_misses);
    }
    return MTH_OK;
}

// ---- --gpus N over a file whose records straddle blocks (METHEOR_SHARD_STRADDLE=1) ---------------------------------------------
// The speculate-then-verify walk of mth_bgzf_decode_straddle one level up.  Every shard scans its own run of blocks on its own context
// from a guessed entry (mth_bgzf_straddle_scan: inflate + record chain, nothing decoded), all at once; the shards then meet once and
// the last to arrive verifies the runs against the serial chain -- run 0 enters at the header's end, run r where run r - 1 leaves, a
// run whose assumed entry differs is scanned again from the true one (mth_bgzf_straddle_rescan: the run's bytes and links are still on
// its context, repair rounds only), an entry at or past a run's end passes on -- which leaves ONE table for the file.  Every shard
// plans from it (mth_host_plan_shard_straddle) and loads its blocks as --region loads such a file.  The inflate is paid twice, scan
// and load: profiles/shard_straddle.md.
struct ShardMeet {                    // the shards' threads meet: the last to arrive runs `last` for all of them
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t gen = 0;
    template <class F> void meet(int world, F &&last) {
        std::unique_lock<std::mutex> lk(mu);
        if (++arrived == world) { last(); arrived = 0; ++gen; cv.notify_all(); }
        else { const uint64_t g = gen; cv.wait(lk, [&] { return gen != g; }); }
    }
};
struct ShardStraddle {
    ShardMeet meet;
    bool aligned_failed = false;      // some shard's aligned plan or load met a record that straddles blocks: every shard takes this route
    bool unsettled = false;           // a scan did not settle within the round bound: the refusal stays
    struct Run { mth_host_straddle_run_t plan; mth_straddle_run_t got; mth_ctx_t *ctx = nullptr; uint32_t rounds = 0; };
    std::vector<Run> runs;
    std::vector<mth_host_straddle_row_t> table;        // a row per block of the file
} g_sx;
static_assert(sizeof(mth_host_straddle_row_t) == sizeof(mth_straddle_row_t) && offsetof(mth_host_straddle_row_t, exit) == offsetof(mth_straddle_row_t, exit),
              "the device writes its rows straight into the host planner's table");

bool shard_straddle_on() { const char *e = getenv("METHEOR_SHARD_STRADDLE"); return e && atoi(e) != 0; }

// run in run order by the last shard to arrive, every scan done
void shard_straddle_verify(const mth_host_bgzf_t &bz) {
    uint64_t entry = bz.header_bytes;            // where the chain enters the run at hand, from the run's first byte
    unsigned n_runs = 0, rescans = 0, rounds = 0;
    for (ShardStraddle::Run &r : g_sx.runs) {
        rounds += r.rounds;
        const uint64_t b0 = r.plan.block_beg, b1 = r.plan.block_end;
        if (b1 == b0) continue;                  // an empty run passes its entry on
        ++n_runs;
        uint64_t run_len = 0;
        for (uint64_t b = b0; b < b1; ++b) run_len += bz.isize[b];
        if (entry >= run_len) {                  // a record that started before the run covers it: nothing starts here
            uint64_t left = entry;
            for (uint64_t b = b0; b < b1; ++b) { left -= bz.isize[b]; g_sx.table[b] = mth_host_straddle_row_t{MTH_HOST_STRADDLE_NO_START, INT32_MIN, INT32_MIN, 0, left}; }
            entry -= run_len;
            continue;
        }
        if (r.got.entry != entry) {
            mth_straddle_info_t info;
            const int rc = mth_bgzf_straddle_rescan(r.ctx, entry, reinterpret_cast<mth_straddle_row_t *>(g_sx.table.data() + b0), &r.got, &info);
            ++rescans;
            rounds += info.rounds;
            if (rc == MTH_ERR_UNALIGNED) { g_sx.unsettled = true; return; }
            if (rc == MTH_ERR_FORMAT) die_decode_format(r.ctx, "corrupt BGZF block or BAM record");
            check(r.ctx, rc);
        }
        if (r.got.exit == MTH_STRADDLE_EXIT_BAD) die("Error reading BAM record. corrupt BGZF block or BAM record");   // block_size < 32 on the verified chain
        entry = r.got.exit;
    }
    if (n_runs && entry != 0) die("Error reading BAM record. corrupt BGZF block or BAM record");       // the file ends inside a record
    if (getenv("METHEOR_TIMING")) fprintf(stderr, "[metheor straddle] shard scan: %u runs, %u scanned again, %u rounds\n", n_runs, rescans, rounds);
}

// -> false: a scan did not settle (the caller refuses the file as before)
bool shard_straddle_load(Input &in, mth_host_bgzf_t bz) {
    const int rank = g_shard.rank, world = g_shard.world;
    ShardStraddle::Run run;
    run.ctx = in.ctx;
    run.got = mth_straddle_run_t{0, 0};
    if (mth_host_plan_straddle_run(in.h, rank, world, &run.plan) != 0) die(mth_host_last_error(in.h));
    std::vector<mth_straddle_row_t> rows((size_t)(run.plan.block_end - run.plan.block_beg));
    bool settled = true;
    if (!rows.empty()) {
        Phase ph("  device inflate + straddle scan");
        const uint64_t b0 = run.plan.block_beg, n = run.plan.ahead_end - b0, base = bz.coff[b0];
        std::vector<uint64_t> rel((size_t)n);
        for (uint64_t k = 0; k < n; ++k) rel[(size_t)k] = bz.coff[b0 + k] - base;
        const uint64_t nbytes = bz.coff[b0 + n - 1] + bz.csize[b0 + n - 1] + 8 - base;      // incl. the last block's CRC32 + ISIZE trailer
        mth_straddle_info_t info;
        const int rc = mth_bgzf_straddle_scan(in.ctx, bz.file + base, nbytes, rel.data(), bz.csize + b0, bz.isize + b0, n, rows.size(), run.plan.entry,
                                              rows.data(), &run.got, &info);
        run.rounds = info.rounds;
        if (rc == MTH_ERR_UNALIGNED) settled = false;
        else if (rc == MTH_ERR_FORMAT) die_decode_format(in.ctx, "corrupt BGZF block or BAM record");
        else check(in.ctx, rc);
    }
    {
        std::lock_guard<std::mutex> lk(g_sx.meet.mu);
        if (g_sx.runs.empty()) {                 // sized by whoever comes first, filled by all
            g_sx.table.assign((size_t)bz.n_blocks, mth_host_straddle_row_t{MTH_HOST_STRADDLE_NO_START, INT32_MIN, INT32_MIN, 0, 0});
            g_sx.runs.resize((size_t)world);
        }
        if (!settled) g_sx.unsettled = true;
        g_sx.runs[(size_t)rank] = run;
        if (!rows.empty()) memcpy(g_sx.table.data() + run.plan.block_beg, rows.data(), rows.size() * sizeof rows[0]);
    }
    g_sx.meet.meet(world, [&] { if (!g_sx.unsettled) shard_straddle_verify(bz); });
    if (g_sx.unsettled) return false;
    if (mth_host_plan_shard_straddle(in.h, g_sx.table.data(), g_sx.table.size(), rank, world, g_shard.halo, &g_shard.plan) != 0) die(mth_host_last_error(in.h));
    bz.n_blocks = g_shard.plan.block_end;
    bz.header_bytes = g_shard.plan.first_byte;
    Phase ph(kStraddlePhase);
    return load_chunks(in, bz, g_shard.plan.block_beg, true, true) == MTH_OK;
}

bool load_bgzf_on_device(Input &in) {
    mth_host_bgzf_t bz;
    if (mth_host_bgzf_blocks(in.h, &bz) != 0) die(mth_host_last_error(in.h));
    const uint64_t all_blocks = bz.n_blocks, file_header = bz.header_bytes;
    uint64_t blk_beg = 0;
    // this shard's run of blocks (+ halo blocks), or the blocks the .bai names for --region, instead of the whole file.  at_record: the
    // region plan that starts at the index's exact record offset inside its first block (blocks that do not start at records)
    auto plan = [&](bool at_record) {
        if (g_shard.region) {
            const int tid = mth_host_ref_tid(in.h, g_shard.region_name.c_str());
            if (tid < 0) die("--region: the BAM header has no reference named '" + g_shard.region_name + "'");
            const char *bai = g_shard.bai.empty() ? nullptr : g_shard.bai.c_str();
            if ((at_record ? mth_host_plan_region_at_record : mth_host_plan_region)(in.h, bai, tid, g_shard.r_beg, g_shard.r_end, g_shard.halo, &g_shard.plan) != 0)
                die(mth_host_last_error(in.h));
        } else {
            const int rc = mth_host_plan_shard(in.h, g_shard.rank, g_shard.world, g_shard.halo, &g_shard.plan);
            if (rc == MTH_HOST_ERR_FORMAT && shard_straddle_on()) return false;       // a run does not start at a record boundary
            if (rc != 0) die(mth_host_last_error(in.h));
        }
        blk_beg = g_shard.plan.block_beg;
        bz.n_blocks = g_shard.plan.block_end;
        bz.header_bytes = g_shard.plan.first_byte;
        return true;
    };
    const bool sharded_straddle = g_shard.world > 1 && shard_straddle_on();
    bool aligned = !g_shard.planned() || plan(false);
    if (aligned) {
        Phase ph("  device inflate + walk + decode");
        aligned = load_chunks(in, bz, blk_beg, false, false) == MTH_OK;
        if (aligned && !sharded_straddle) return true;
    }
    if (sharded_straddle) {
        // the aligned planner can accept such a file by accident (or have nothing to load) where its neighbour's fails: the route is
        // the run's, not the shard's, so the shards agree on it first
        { std::lock_guard<std::mutex> lk(g_sx.meet.mu); if (!aligned) g_sx.aligned_failed = true; }
        g_sx.meet.meet(g_shard.world, [] {});
        if (!g_sx.aligned_failed) return true;
        if (aligned) check(in.ctx, mth_reset(in.ctx));        // what this shard decoded belongs to a plan the others could not follow
        bz.n_blocks = all_blocks; bz.header_bytes = file_header;
        return shard_straddle_load(in, bz);
    }
    const char *e = getenv("METHEOR_DEVICE_STRADDLE");
    if (g_shard.world > 1 || !(g_shard.region || (e && atoi(e) != 0))) return false;
    bz.n_blocks = all_blocks; bz.header_bytes = file_header;
    if (g_shard.region) plan(true);
    Phase ph(kStraddlePhase);
    return load_chunks(in, bz, blk_beg, true, g_shard.region) == MTH_OK;
}

bool batch_decoded(Input &in, const std::vector<int32_t> &tids, const std::vector<uint64_t> &rb, const std::vector<uint64_t> &re,
                   uint32_t n_runs, uint32_t flags);

bool load_on_device(Input &in, const char *cpg_set, CtxFuture &cf) {
    const uint64_t *keys = nullptr;
    uint64_t n_keys = 0;
    if (cpg_set && mth_host_cpg_set_keys(in.h, cpg_set, &keys, &n_keys) != 0) { cf.wait(); die(mth_host_last_error(in.h)); }   // readutil.rs:356
    {
        mth_host_bgzf_t bz;                      // builds (and caches) the block table while the context is being created
        if (!getenv("METHEOR_HOST_INFLATE") && mth_host_bgzf_blocks(in.h, &bz) != 0) { cf.wait(); die(mth_host_last_error(in.h)); }
    }
    // --genome: the FASTA is read here, while the context is being created; the first record's paired flag is the FILE's
    // (bamutil.rs:27-37), whatever part of it this shard / region loads
    int first_flag = -1;
    if (!g_genome.path.empty()) {
        genome_read_once(in.h, [&] { cf.wait(); });
        if (mth_host_first_flag(in.h, &first_flag) != 0) { cf.wait(); die(mth_host_last_error(in.h)); }
    }
    // (touching the mapped file's pages from 16 threads while the HIP runtime starts was measured: it slows the start-up
    // it competes with and the copies gain nothing, profiles/r02_e2e.md)
    in.ctx = cf.get();
    if (!g_genome.path.empty()) {
        Phase ph("  genome -> device");
        genome_upload(in.ctx, in.h, g_genome, [] {});
        check(in.ctx, mth_decode_set_genome(in.ctx, 1, first_flag >= 0 && (first_flag & 1)));
    }
    if (g_modtags) check(in.ctx, mth_decode_set_modtags(in.ctx, 1, g_mm_threshold));
    if (cpg_set) check(in.ctx, mth_decode_set_cpg_filter(in.ctx, keys, n_keys, 1));
    check(in.ctx, mth_decode_set_xm_min_mapq(in.ctx, (uint32_t)g_shard.xm_min_mapq));
    const bool on_device = !getenv("METHEOR_HOST_INFLATE") && load_bgzf_on_device(in);
    if (!on_device && g_shard.planned()) die("--gpus N / --region need the device load path (a coordinate-sorted BAM whose records do not straddle BGZF blocks)");
    if (!on_device) {
        StreamState st;
        st.ctx = in.ctx;
        Phase ph("  inflate + device record decode");
        const int rc = mth_host_decode_stream(in.h, window_to_device, &st);
        if (st.rc == MTH_ERR_FORMAT) die_decode_format(in.ctx, "corrupt BAM record");
        if (st.rc != MTH_OK) check(in.ctx, st.rc);
        if (rc != 0) die(mth_host_last_error(in.h));
        if (st.first) {   // no record at all: an empty decode
            mth_decoded_t d;
            check(in.ctx, mth_decode_records(in.ctx, nullptr, 0, nullptr, 0, MTH_MEM_HOST, 0, &d));
        }
    }
    Phase ph2("  contig ranges");
    // one run of equal tid per contig in a coordinate-sorted file; anything else the batches cannot hold as it is
    const uint32_t cap = (uint32_t)std::max(1, mth_host_n_refs(in.h)) + 1;
    std::vector<int32_t> tids(cap);
    std::vector<uint64_t> rb(cap), re(cap);
    uint32_t n_runs = 0, flags = 0;
    check(in.ctx, mth_decoded_contigs(in.ctx, cap, tids.data(), rb.data(), re.data(), &n_runs, &flags));
    {
        // not coordinate-sorted / contigs not grouped: the order-free measures sort the decoded stream where it is, on the device
        // (mth_decoded_sort); the others go on to the host path, which says why it refuses
        bool regroup = n_runs > cap || (flags & 4u);
        for (uint32_t k = 0; k < std::min(n_runs, cap) && !regroup; ++k)
            for (uint32_t j = 0; j < k; ++j) if (tids[j] == tids[k]) regroup = true;
        if (regroup && g_shard.order_free && !(flags & 3u) && !g_shard.planned()) {
            Phase ps("  device sort by (tid, start)");
            check(in.ctx, mth_decoded_sort(in.ctx));
            check(in.ctx, mth_decoded_contigs(in.ctx, cap, tids.data(), rb.data(), re.data(), &n_runs, &flags));
        } else if (regroup && !g_shard.order_free && !g_shard.planned()) {
            // pdr / mhl / fdrp / qfdrp finalise sites as the stream moves past them: on such input their result is a function of the
            // record order itself (pdr.rs:139-178, mhl.rs:155-173, fdrp.rs:197-223), which the decoded stream still has -- replayed as
            // it is (mth_fileorder.hip), no batches
            in.file_order = true;
            in.device = true;
            in.dec_flags = flags;
            return true;
        }
    }
    return batch_decoded(in, tids, rb, re, n_runs, flags);
}

// the decoded stream's contig runs (mth_decoded_contigs) as the batches of the device path: false when the batches cannot hold them
bool batch_decoded(Input &in, const std::vector<int32_t> &tids, const std::vector<uint64_t> &rb, const std::vector<uint64_t> &re,
                   uint32_t n_runs, uint32_t flags) {
    const uint32_t cap = (uint32_t)tids.size();
    if (flags || n_runs > cap) return false;                       // unaligned / contig-less records, or contigs not grouped
    for (uint32_t k = 0; k < n_runs; ++k) {
        for (const Contig &c : in.contigs) if (c.tid == tids[k]) return false;   // the host path reports it
        int32_t reg_beg = 0, reg_end = -1;
        if (g_shard.planned()) {      // the part of this contig inside the shard's / region's interval [(tid_beg, pos_beg), (tid_end, pos_end))
            const mth_host_shard_t &pl = g_shard.plan;
            if (tids[k] < pl.tid_beg || tids[k] > pl.tid_end) continue;               // halo reads of a neighbour's contig
            if (tids[k] == pl.tid_beg) reg_beg = pl.pos_beg;
            if (tids[k] == pl.tid_end && pl.pos_end != INT32_MAX) { reg_end = pl.pos_end; if (reg_end <= reg_beg) continue; }
        }
        in.contigs.emplace_back();
        Contig &c = in.contigs.back();
        c.tid = tids[k]; c.r0 = rb[k]; c.r1 = re[k]; c.n_reads = (size_t)(re[k] - rb[k]); c.n_cpgs = 0;
        c.region_beg = reg_beg; c.region_end = reg_end;
    }
    // Several contigs per batch (include/metheor_hip.h, "contig groups"): every pass pays its fixed costs per batch, and a human BAM
    // has 24 to a few thousand contigs.  The library shifts the decoded positions into one virtual coordinate space per group and maps
    // the rows back at the fetch, so nothing below this line knows.  Not under a shard / region plan (those own parts of contigs);
    // METHEOR_GROUP=0 keeps one batch per contig (A/B, tests).
    // A contig that holds a call at position -1 (a record at 0 under a shifted flag calling on its first base) is shifted too, also when
    // it is the only one, under METHEOR_GROUP=0 and under a region plan: one group per contig then (mth_decoded_group_each), which leaves
    // every other contig as it is.
    const bool merge = !g_shard.planned() && in.contigs.size() > 1 && !(getenv("METHEOR_GROUP") && atoi(getenv("METHEOR_GROUP")) == 0);
    if (!in.contigs.empty()) {
        std::unique_ptr<Phase> pg(merge ? new Phase("  contig groups") : nullptr);
        const uint32_t nc = (uint32_t)in.contigs.size();
        std::vector<int32_t> gt(nc), bt(nc);
        std::vector<uint64_t> gb(nc), ge(nc);
        std::vector<uint32_t> first((size_t)nc + 1);
        for (uint32_t k = 0; k < nc; ++k) { gt[k] = in.contigs[k].tid; gb[k] = in.contigs[k].r0; ge[k] = in.contigs[k].r1; }
        uint32_t ng = 0;
        check(in.ctx, (merge ? mth_decoded_group : mth_decoded_group_each)(in.ctx, nc, gt.data(), gb.data(), ge.data(), &ng, first.data(), bt.data()));
        if (ng) {
            std::vector<Contig> grouped((size_t)ng);
            for (uint32_t g = 0; g < ng; ++g) {
                Contig &c = grouped[g];
                c.tid = bt[g]; c.r0 = gb[first[g]]; c.r1 = ge[first[g + 1] - 1]; c.n_reads = (size_t)(c.r1 - c.r0); c.n_cpgs = 0;
                c.region_beg = 0; c.region_end = -1;
                if (!merge) {     // one contig each: its region stays, in shifted positions where the contig was shifted (from BASE - 1: the site at -1)
                    const Contig &o = in.contigs[first[g]];
                    const int32_t up = bt[g] <= -2 ? MTH_GROUP_MINUS_ONE_BASE : 0;
                    c.region_beg = o.region_beg + up - (up && o.region_beg == 0 ? 1 : 0);
                    c.region_end = o.region_end < 0 ? -1 : (int32_t)std::min<int64_t>((int64_t)o.region_end + up, INT32_MAX);
                }
            }
            in.contigs.swap(grouped);
        }
    }
    in.device = true;
    return true;
}

// LPMD, ME and PM keep no per-site state that a later read could flush (lpmd.rs:175-200, me.rs:106-125, pm.rs:101-121 iterate the
// records in file order into hash maps that are only read at the end): their results do not depend on the order of the
// records, and the reference accepts any BAM.  For those subcommands an input that is not coordinate-sorted / not grouped by
// contig is sorted here, stably by (tid, start), and then batched like any other.  PDR, MHL, FDRP and qFDRP finalise sites as
// the stream moves past them (pdr.rs:160-177, mhl.rs:162-173, fdrp.rs:206-218): their output on unsorted input is a function
// of the record order itself, which batches cut by contig do not carry -- those subcommands keep refusing it, loudly.
bool reads_in_order(const int32_t *tid, const int32_t *st, int64_t n) {
    // Records without an aligned base never enter a batch: not looked at.  Records without a contig (a sorted BAM keeps them at
    // its end) do not either, but the batching loop below cuts the contigs' runs at them: one BETWEEN two placed records -- tids
    // 0, -1, 0 re-open contig 0's run; 0, -1, 1 is harmless but not what a sort gives -- counts as out of order, so that the
    // order-free measures sort the file (the stable sort puts such records first, where they are skipped and counted) instead of
    // dying on "not grouped by contig".
    int64_t p = -1;
    bool loose_seen = false;
    for (int64_t i = 0; i < n; ++i) {
        if (tid[i] < 0) { loose_seen = p >= 0; continue; }
        if (loose_seen) return false;
        if (st[i] < 0) continue;
        if (p >= 0 && (tid[i] < tid[p] || (tid[i] == tid[p] && st[i] < st[p]))) return false;
        p = i;
    }
    return true;
}

// group_ctx: the context the batches of a host-only load go to, when the caller has one already (`all`)
Input load(const std::string &path, const char *cpg_set, bool host_only = false, mth_ctx_t *group_ctx = nullptr) {
    Phase ph_all("load: open+decode+batch");
    Input in;
    char err[1024];
    const bool try_device = !getenv("METHEOR_HOST_DECODE") && !host_only;
    if (!try_device && g_shard.planned()) die("--gpus N / --region need the device load path (METHEOR_HOST_DECODE is set)");
    if (!try_device && !g_genome.path.empty()) die(kNoHostGenome);
    if (!try_device && g_modtags) die(kNoHostModtags);
    CtxFuture cf;
    if (try_device) cf.start();
    if (mth_host_open(path.c_str(), &in.h, err, sizeof err) != 0) { cf.wait(); die(err); }    // bamutil.rs:7-9
    if (try_device) {
        if (load_on_device(in, cpg_set, cf)) return in;
        if (g_shard.planned()) die("--gpus N / --region need the device load path (coordinate-sorted input, contigs grouped, records inside BGZF blocks)");
        if (!g_genome.path.empty()) die(kNoHostGenome);
        if (g_modtags) die(kNoHostModtags);
        in.contigs.clear();
    }
    {
        Phase ph("  host decode (BGZF+BAM+XM)");
        mth_host_set_xm_min_mapq(in.h, g_shard.xm_min_mapq);
        if (mth_host_decode(in.h, cpg_set) != 0) die(mth_host_last_error(in.h));
    }
    Phase ph2("  contig batches");
    const int64_t n = mth_host_n_reads(in.h);
    const int32_t *tid = mth_host_read_tid(in.h), *st = mth_host_read_start(in.h), *en = mth_host_read_end(in.h);
    const uint8_t *mq = mth_host_read_mapq(in.h);
    const uint64_t *off = mth_host_cpg_off(in.h);
    const uint32_t *pos = mth_host_cpg_pos(in.h);
    const uint16_t *rel = mth_host_cpg_rel(in.h);
    if (!reads_in_order(tid, st, n)) {
        if (!g_shard.order_free)
            die("input BAM is not coordinate-sorted (or not grouped by contig), and it had to be decoded on the host (records that straddle "
                "BGZF blocks, or METHEOR_HOST_DECODE): pdr, mhl, fdrp and qfdrp finalise a CpG as the reads move past it (pdr.rs:160-177, "
                "mhl.rs:162-173, fdrp.rs:206-218), so their output on such input depends on the record order itself, which only the device "
                "decode path replays (mth_fileorder_run) -- sort the file (samtools sort).  lpmd, me and pm take any order.");
        Phase ps("  sort by (tid, start)");
        std::vector<int64_t> perm((size_t)n);
        for (int64_t i = 0; i < n; ++i) perm[(size_t)i] = i;
        std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) { return tid[x] != tid[y] ? tid[x] < tid[y] : st[x] < st[y]; });
        in.s_tid.resize((size_t)n); in.s_start.resize((size_t)n); in.s_end.resize((size_t)n); in.s_mapq.resize((size_t)n);
        in.s_off.assign((size_t)n + 1, 0);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t r = perm[(size_t)i];
            in.s_tid[(size_t)i] = tid[r]; in.s_start[(size_t)i] = st[r]; in.s_end[(size_t)i] = en[r]; in.s_mapq[(size_t)i] = mq[r];
            in.s_off[(size_t)i + 1] = in.s_off[(size_t)i] + (off[r + 1] - off[r]);
        }
        in.s_pos.resize((size_t)in.s_off[(size_t)n]); in.s_rel.resize((size_t)in.s_off[(size_t)n]);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t r = perm[(size_t)i];
            std::copy(pos + off[r], pos + off[r + 1], in.s_pos.begin() + (ptrdiff_t)in.s_off[(size_t)i]);
            std::copy(rel + off[r], rel + off[r + 1], in.s_rel.begin() + (ptrdiff_t)in.s_off[(size_t)i]);
        }
        tid = in.s_tid.data(); st = in.s_start.data(); en = in.s_end.data(); mq = in.s_mapq.data();
        off = in.s_off.data(); pos = in.s_pos.data(); rel = in.s_rel.data();
    }
    for (int64_t i = 0; i < n;) {
        int64_t e = i;
        bool loose = false;
        while (e < n && tid[e] == tid[i]) { loose |= st[e] < 0; ++e; }
        if (tid[i] < 0) { in.unbatched_mapq.insert(in.unbatched_mapq.end(), mq + i, mq + e); i = e; continue; }   // records without a contig never enter a batch
        for (const Contig &c : in.contigs)
            if (c.tid == tid[i]) die("input BAM is not grouped by contig (coordinate-sorted input is required on the MI355X path)");
        in.contigs.emplace_back();
        Contig &c = in.contigs.back();
        c.tid = tid[i];
        if (!loose) {
            c.start = st + i; c.end = en + i; c.mapq = mq + i; c.pos = pos + off[i]; c.rel = rel + off[i];
            c.n_reads = (size_t)(e - i); c.n_cpgs = (size_t)(off[e] - off[i]);
            c.off.resize(c.n_reads + 1);
            int32_t ms = 0;
            if (off[e] - off[i] >= (1ull << 32) || (uint64_t)(e - i) >= (1ull << 32) - 1) die("metheor (MI355X path): a contig with 2^32 or more reads / CpG calls does not fit one batch on the host-decode path");
            for (int64_t r = i; r < e; ++r) { c.off[(size_t)(r - i)] = (uint32_t)(off[r] - off[i]); ms = std::max(ms, en[r] - st[r] + 1); c.max_end = std::max(c.max_end, en[r]); }
            c.off[c.n_reads] = (uint32_t)(off[e] - off[i]);
            c.max_span = ms;
        } else {
            c.off.push_back(0);
            for (int64_t r = i; r < e; ++r) {
                if (st[r] < 0) { in.unbatched_mapq.push_back(mq[r]); continue; }   // no aligned base: no CpG, no position
                c.o_start.push_back(st[r]); c.o_end.push_back(en[r]); c.o_mapq.push_back(mq[r]);
                for (uint64_t k = off[r]; k < off[r + 1]; ++k) { c.o_pos.push_back(pos[k]); c.o_rel.push_back(rel[k]); }
                if (c.o_pos.size() >= (1ull << 32)) die("metheor (MI355X path): a contig with 2^32 or more CpG calls does not fit one batch on the host-decode path");
                c.off.push_back((uint32_t)c.o_pos.size());
                c.max_span = std::max(c.max_span, en[r] - st[r] + 1);
                c.max_end = std::max(c.max_end, en[r]);
            }
            c.start = c.o_start.data(); c.end = c.o_end.data(); c.mapq = c.o_mapq.data(); c.pos = c.o_pos.data(); c.rel = c.o_rel.data();
            c.n_reads = c.o_start.size(); c.n_cpgs = c.o_pos.size();
        }
        // a call at position -1 (the word 0x7fffffff; the first call of a read at 0): no batch may carry it -- the contig is copied
        // MTH_GROUP_MINUS_ONE_BASE positions up and goes in as a contig group of one (make_batch), the fetch maps its rows back
        for (size_t r = 0; r < c.n_reads && c.start[r] == 0 && !c.lifted; ++r)
            c.lifted = c.off[r + 1] > c.off[r] && (c.pos[c.off[r]] & 0x7fffffffu) == 0x7fffffffu;
        if (c.lifted) {
            if (c.o_start.empty()) {
                c.o_start.assign(c.start, c.start + c.n_reads); c.o_end.assign(c.end, c.end + c.n_reads); c.o_mapq.assign(c.mapq, c.mapq + c.n_reads);
                c.o_pos.assign(c.pos, c.pos + c.n_cpgs); c.o_rel.assign(c.rel, c.rel + c.n_cpgs);
            }
            for (int32_t &v : c.o_start) v += MTH_GROUP_MINUS_ONE_BASE;
            for (int32_t &v : c.o_end) v += MTH_GROUP_MINUS_ONE_BASE;
            for (uint32_t &w : c.o_pos) w = ((w + (uint32_t)MTH_GROUP_MINUS_ONE_BASE) & 0x7fffffffu) | (w & 0x80000000u);
            c.start = c.o_start.data(); c.end = c.o_end.data(); c.mapq = c.o_mapq.data(); c.pos = c.o_pos.data(); c.rel = c.o_rel.data();
            c.max_end += MTH_GROUP_MINUS_ONE_BASE;
        }
        i = e;
    }
    for (Contig &c : in.contigs) {
        if (!c.lifted) continue;
        if (!in.ctx) in.ctx = group_ctx ? group_ctx : make_ctx();
        const int64_t voff = MTH_GROUP_MINUS_ONE_BASE;
        check(in.ctx, mth_group_define(in.ctx, 1, &c.tid, &voff, &c.group));
    }
    return in;
}

mth_batch_t make_batch(const Input &in, const Contig &c) {
    mth_batch_t b;
    memset(&b, 0, sizeof b);
    if (in.device) {
        // a whole contig (or a shard's last piece of it) ends where its reads end, not at the header's LN:
        // the reference has no notion of LN in this path and emits sites beyond it
        check(in.ctx, mth_decoded_batch(in.ctx, c.r0, c.r1, c.tid, c.region_beg, c.region_end >= 0 ? c.region_end : -1, &b));
        if (g_shard.planned() && (int64_t)b.max_span + 202 > g_shard.halo)
            die("an alignment spans " + std::to_string(b.max_span) + " bp: set METHEOR_SHARD_HALO to at least " + std::to_string(b.max_span + 202));
        return b;
    }
    b.tid = c.lifted ? c.group : c.tid;
    b.region_beg = 0;
    b.region_end = (int32_t)std::min<int64_t>((int64_t)c.max_end + 2, INT32_MAX);      // to the end of the data, not the header's LN
    b.max_span = c.max_span;
    b.n_reads = (uint32_t)c.n_reads;
    b.n_cpgs = (uint32_t)c.n_cpgs;
    b.mem = MTH_MEM_HOST;
    b.read_start = c.start; b.read_end = c.end; b.read_mapq = c.mapq;
    b.cpg_off = c.off.data(); b.cpg_pos = c.pos; b.cpg_rel16 = c.rel;
    return b;
}

void submit(mth_ctx_t *ctx, const Input &in, const mth_pdr_lpmd_params_t &p) {
    for (const Contig &c : in.contigs) {
        const mth_batch_t b = make_batch(in, c);
        check(ctx, mth_pdr_lpmd_accumulate(ctx, &b, &p));
    }
}

// TSV lines are assembled by hand into a large buffer (one write per ~4 MiB instead of one per line)
struct LineWriter {
    FILE *f;
    std::vector<char> buf;
    explicit LineWriter(FILE *file) : f(file) { buf.reserve(4u << 20); }
    void str(const char *s) { buf.insert(buf.end(), s, s + strlen(s)); }
    void ch(char c) { buf.push_back(c); }
    void i64(long long v) { char t[24]; const int n = snprintf(t, sizeof t, "%lld", v); buf.insert(buf.end(), t, t + n); }
    void u32(uint32_t v) {
        char t[12]; int n = 0;
        do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
        while (n) buf.push_back(t[--n]);
    }
    void i32(int32_t v) { if (v < 0) { ch('-'); u32((uint32_t)(-(int64_t)v)); } else u32((uint32_t)v); }
    void f32(float v) { char t[64]; const int n = mth_host_format_f32(v, t); buf.insert(buf.end(), t, t + n); }
    void eol() { ch('\n'); if (f && buf.size() > (4u << 20) - 256) flush(); }   // f == nullptr: an in-memory part
    void flush() { if (!buf.empty() && fwrite(buf.data(), 1, buf.size(), f) != buf.size()) die("Error writing to output file."); buf.clear(); }
};

// n rows -> f: contiguous row ranges are formatted by several threads into their own buffers (the f32 shortest
// round-trip formatting is most of a 700 k-line TSV's cost) and written out in row order
template <class Row>
void write_rows(FILE *f, uint64_t n, Row &&row) {
    int nt = (int)std::thread::hardware_concurrency();
    if (const char *e = getenv("METHEOR_THREADS")) { const int k = atoi(e); if (k >= 1 && k <= 1024) nt = k; }
    nt = std::max(1, std::min(nt / g_shard.world, 32));      // the shards of a --gpus N run format side by side
    if (n < 50000) nt = 1;
    std::vector<LineWriter> parts;
    parts.reserve((size_t)nt);
    for (int t = 0; t < nt; ++t) parts.emplace_back(nt == 1 ? f : nullptr);
    auto work = [&](int t) {
        const uint64_t r0 = n * (uint64_t)t / (uint64_t)nt, r1 = n * (uint64_t)(t + 1) / (uint64_t)nt;
        for (uint64_t i = r0; i < r1; ++i) row(parts[(size_t)t], i);
    };
    if (nt == 1) { work(0); parts[0].flush(); return; }
    // (every thread writing its own part with pwrite at its offset was measured SLOWER than this ordered append on tmpfs:
    // 22 against 15 ms for the 25-MB PDR table, profiles/r02_e2e.md)
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back(work, t);
    for (auto &x : th) x.join();
    for (auto &w : parts) { w.f = f; w.flush(); }
}

FILE *open_file(const std::string &path) {
    FILE *f = fopen(path.c_str(), "wb");   // create + truncate (pdr.rs:95-101)
    if (!f) die("called `Result::unwrap()` on an `Err` value: cannot open output file " + path + ": " + strerror(errno));
    return f;
}

// one shard of several: its rows are collected in memory (main() concatenates the parts in shard order)
FILE *open_output(const std::string &path, bool pairs = false) {
    if (g_shard.world > 1) {
        FILE *f = pairs ? open_memstream(&g_part->pairs, &g_part->pairs_len) : open_memstream(&g_part->out, &g_part->out_len);
        if (!f) die("cannot allocate an output part");
        return f;
    }
    FILE *f = open_file(path);
    static char buf[1 << 20];
    setvbuf(f, buf, _IOFBF, sizeof buf);
    return f;
}

// LPMDResult's counters are genome-wide: the shards meet, the last one to arrive runs the RCCL all-reduce for all
// of them (mth_allreduce_lpmd; lpmd.rs:11-12, 51-55), and every context then holds the totals
void gang_allreduce_lpmd(mth_ctx_t *ctx) {
    std::unique_lock<std::mutex> lk(g_gang.mu);
    g_gang.ctxs.resize((size_t)g_shard.world);
    g_gang.ctxs[(size_t)g_shard.rank] = ctx;
    if (++g_gang.arrived == g_shard.world) {
        g_gang.rc = mth_allreduce_lpmd(g_gang.ctxs.data(), g_shard.world);
        g_gang.done = true;
        g_gang.cv.notify_all();
    } else {
        g_gang.cv.wait(lk, [] { return g_gang.done; });
    }
    if (g_gang.rc != MTH_OK) check(g_gang.ctxs[0], g_gang.rc);
}

// ---- the measures' TSV writers (shared by the single commands and `all`) -----------------------------------------------------

// pdr / mhl / fdrp / qfdrp of an input that is not coordinate-sorted: the stream replayed in file order on the device
// (mth_fileorder.hip); which: 0 = the PDR line (pdr.rs:102-116), 1 = value v0 (mhl.rs:114-132, fdrp.rs:162-173), 2 = value v1 (qfdrp.rs:174-185).
// FDRP's replay gives both values: `all` passes both paths (path2: the qFDRP file).
void file_order_write(Input &in, mth_ctx_t *ctx, const mth_fileorder_params_t &fp, int which, const std::string &path,
                      const std::string *path2 = nullptr) {
    uint64_t n = 0;
    {
        Phase ph("file-order replay (kernels, sync)");
        check(ctx, mth_fileorder_run(ctx, &fp));
        check(ctx, mth_fileorder_fetch(ctx, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    }
    Phase ph3("fetch + TSV write");
    std::vector<int32_t> tid(n), pos(n);
    std::vector<float> v0(n), v1(n);
    std::vector<uint32_t> c0(n), c1(n);
    check(ctx, mth_fileorder_fetch(ctx, &n, tid.data(), pos.data(), v0.data(), v1.data(), c0.data(), c1.data()));
    auto one = [&](const std::string &out, int w_) {
        FILE *f = open_output(out);
        write_rows(f, n, [&](LineWriter &w, uint64_t i) {
            w.str(mth_host_ref_name(in.h, tid[i])); w.ch('\t'); w.i32(pos[i]); w.ch('\t'); w.i32(pos[i] + 2); w.ch('\t');
            if (w_ == 0) { w.f32(v0[i]); w.ch('\t'); w.u32(c0[i]); w.ch('\t'); w.u32(c1[i]); }
            else w.f32(w_ == 2 ? v1[i] : v0[i]);
            w.eol();
        });
        if (fclose(f) != 0) die("Error writing to output file.");
    };
    if (!path.empty()) one(path, which);
    if (path2) one(*path2, 2);
}

int run_file_order(const Args &a, Input &in, mth_ctx_t *ctx, const mth_fileorder_params_t &fp, int which) {
    file_order_write(in, ctx, fp, which, a.s.at("output"));
    return finish(ctx, in.h);
}

// pdr.rs:102-116: the PDR rows accumulated so far
void pdr_write(mth_ctx_t *ctx, const Input &in, const std::string &path) {
    uint64_t n = 0;
    check(ctx, mth_pdr_count(ctx, &n));
    Phase ph3("fetch + TSV write");
    // the five columns in one page-locked allocation (device-to-host at the link's rate; nothing to zero-fill)
    void *pin = nullptr;
    check(ctx, mth_result_buffer_alloc(ctx, (size_t)n * 20, &pin));
    int32_t *tid = (int32_t *)pin, *pos = tid + n;
    float *pdr = (float *)(pos + n);
    uint32_t *nc = (uint32_t *)(pdr + n), *nd = nc + n;
    { Phase pf("  fetch"); check(ctx, mth_pdr_fetch(ctx, tid, pos, pdr, nc, nd)); }
    Phase pw("  format + write");
    FILE *f = open_output(path);
    write_rows(f, n, [&](LineWriter &w, uint64_t i) {   // pdr.rs:102-116
        w.str(mth_host_ref_name(in.h, tid[i])); w.ch('\t'); w.i32(pos[i]); w.ch('\t'); w.i32(pos[i] + 2); w.ch('\t');
        w.f32(pdr[i]); w.ch('\t'); w.u32(nc[i]); w.ch('\t'); w.u32(nd[i]); w.eol();
    });
    if (fclose(f) != 0) die("Error writing to output file.");
    if (getenv("METHEOR_TEARDOWN")) check(ctx, mth_result_buffer_free(ctx, pin));   // (unpinning is a few ms: left to the process's end otherwise)
}

// lpmd.rs:145-147: the LPMD line, after the records that entered no batch are counted (and, --gpus N, the counters all-reduced)
void lpmd_write(mth_ctx_t *ctx, const Input &in, const std::string &input, uint8_t min_qual, const std::string &path) {
    if (!in.unbatched_mapq.empty()) {                            // lpmd.rs:176-179: every record counts, also those without a position
        uint64_t nv = 0;
        for (uint8_t q : in.unbatched_mapq) nv += q >= min_qual ? 1u : 0u;
        check(ctx, mth_lpmd_add_unbatched(ctx, in.unbatched_mapq.size(), nv));
    }
    if (g_shard.world > 1) gang_allreduce_lpmd(ctx);             // every shard now holds the genome-wide counters
    int64_t g[4] = {0, 0, 0, 0};
    float lp = 0.f;
    check(ctx, mth_lpmd_global(ctx, g, &lp));
    if (getenv("METHEOR_DEBUG_COUNTS")) fprintf(stderr, "[metheor counts] n_concordant=%lld n_discordant=%lld n_read=%lld n_valid_read=%lld\n", (long long)g[0], (long long)g[1], (long long)g[2], (long long)g[3]);
    // records that never enter a batch only move n_read / n_valid_read (not part of the TSV)
    FILE *f = open_output(path);
    char fb[64];
    mth_host_format_f32(lp, fb);
    if (g_shard.rank == 0) fprintf(f, "name\tlpmd\n%s\t%s\n", input.c_str(), fb);   // lpmd.rs:145-147
    if (fclose(f) != 0) die("Error writing to output file.");
}

// lpmd.rs:149-151, 89-122: the per-pair table accumulated so far
void lpmd_pairs_write(mth_ctx_t *ctx, const Input &in, const std::string &path) {
    uint64_t n = 0;
    check(ctx, mth_lpmd_pairs_fetch(ctx, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    std::vector<int32_t> tid(n), p1(n), p2(n);
    std::vector<float> v(n);
    std::vector<uint32_t> nc(n), nd(n);
    check(ctx, mth_lpmd_pairs_fetch(ctx, &n, tid.data(), p1.data(), p2.data(), v.data(), nc.data(), nd.data()));
    FILE *g = open_output(path, true);
    if (g_shard.rank == 0) fprintf(g, "chrom\tcpg1\tcpg2\tlpmd\tn_concordant\tn_discordant\n");
    fflush(g);
    write_rows(g, n, [&](LineWriter &w, uint64_t i) {
        w.str(mth_host_ref_name(in.h, tid[i])); w.ch('\t'); w.i32(p1[i]); w.ch('\t'); w.i32(p2[i]); w.ch('\t');
        w.f32(v[i]); w.ch('\t'); w.u32(nc[i]); w.ch('\t'); w.u32(nd[i]); w.eol();
    });
    if (fclose(g) != 0) die("Error writing to output file.");
}

// ---- lpmd --intervals: LPMD per interval of a BED file -------------------------------------------------------
// Read by main() before any device or output is touched; every shard of a --gpus N run reduces its own rows for all of them.
struct Intervals {
    std::string path, out_path, mhl_path, pdr_path;      // out_path: the per-interval LPMD table, mhl_path / pdr_path: the per-interval MHL / PDR table
    std::string me_path, pm_path;                        // the per-interval ME / PM table (one pass counts for both)
    std::vector<std::string> chrom, name;
    std::vector<int32_t> tid, beg, end;
    bool on() const { return !out_path.empty(); }
    bool mhl_on() const { return !mhl_path.empty(); }
    bool pdr_on() const { return !pdr_path.empty(); }
    bool quartet_on() const { return !me_path.empty() || !pm_path.empty(); }
    // one of the tables, a row per BED line: chrom, start, end, name, then the measure's own columns (`header`; row(w, i) writes them)
    template <class Row>
    void table(const std::string &table_path, const char *header, Row &&row) const {
        FILE *f = open_file(table_path);
        fprintf(f, "chrom\tstart\tend\tname\t%s\n", header);
        LineWriter w(f);
        for (size_t i = 0; i < tid.size(); ++i) {
            w.str(chrom[i].c_str()); w.ch('\t'); w.i32(beg[i]); w.ch('\t'); w.i32(end[i]); w.ch('\t'); w.str(name[i].c_str()); w.ch('\t');
            row(w, i); w.eol();
        }
        w.flush();
        if (fclose(f) != 0) die("Error writing to output file.");
    }
} g_intervals;

// BED: tab-separated, chrom start end [name [...]], 0-based half-open; empty lines and '#' / track / browser lines are skipped
void intervals_read(const mth_host_t *h) {
    Intervals &iv = g_intervals;
    FILE *f = fopen(iv.path.c_str(), "rb");
    if (!f) die("Error opening intervals file " + iv.path + ": " + strerror(errno));
    std::string text;
    char chunk[1 << 16];
    for (size_t k; (k = fread(chunk, 1, sizeof chunk, f)) > 0;) text.append(chunk, k);
    fclose(f);
    auto bad = [&](size_t line_no, const std::string &why) { die("Error reading intervals file " + iv.path + ": line " + std::to_string(line_no) + ": " + why); };
    auto number = [&](const std::string &v, size_t line_no, const char *what) -> int32_t {
        if (v.empty() || v.size() > 10 || v.find_first_not_of("0123456789") != std::string::npos)
            bad(line_no, std::string(what) + " '" + v + "' is not a number in 0..=2147483647");
        const long long x = strtoll(v.c_str(), nullptr, 10);
        if (x > INT32_MAX) bad(line_no, std::string(what) + " '" + v + "' is not a number in 0..=2147483647");
        return (int32_t)x;
    };
    size_t line_no = 0;
    for (size_t p = 0; p < text.size();) {
        size_t e = text.find('\n', p);
        if (e == std::string::npos) e = text.size();
        std::string line = text.substr(p, e - p);
        p = e + 1;
        ++line_no;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#' || line.rfind("track", 0) == 0 || line.rfind("browser", 0) == 0) continue;
        std::vector<std::string> col;
        for (size_t c = 0;;) {
            const size_t t = line.find('\t', c);
            col.push_back(line.substr(c, t == std::string::npos ? std::string::npos : t - c));
            if (t == std::string::npos || col.size() == 4) break;
            c = t + 1;
        }
        if (col.size() < 3) bad(line_no, "fewer than 3 tab-separated columns");
        const int32_t b = number(col[1], line_no, "start"), en = number(col[2], line_no, "end");
        if (b > en) bad(line_no, "start " + col[1] + " is beyond end " + col[2]);
        const int tid = mth_host_ref_tid(h, col[0].c_str());
        if (tid < 0) bad(line_no, "the input's header has no reference named '" + col[0] + "'");
        iv.chrom.push_back(col[0]); iv.name.push_back(col.size() > 3 && !col[3].empty() ? col[3] : ".");
        iv.tid.push_back(tid); iv.beg.push_back(b); iv.end.push_back(en);
    }
}

// lpmd (lpmd.rs:51-55 over the interval's own counters), n_concordant, n_discordant
void intervals_write(const std::vector<int64_t> &nc, const std::vector<int64_t> &nd) {
    g_intervals.table(g_intervals.out_path, "lpmd\tn_concordant\tn_discordant", [&](LineWriter &w, size_t i) {
        w.f32(mth_lpmd_from_counts(nc[i], nd[i])); w.ch('\t'); w.i64(nc[i]); w.ch('\t'); w.i64(nd[i]);
    });
}

// the pairs table accumulated on this context, reduced by interval on the device (a shard of several: its sums go to main(), which
// adds the shards' -- a pair is owned by the shard that holds cpg1 -- and writes the file)
void lpmd_intervals_write(mth_ctx_t *ctx) {
    const Intervals &iv = g_intervals;
    const size_t n = iv.tid.size();
    std::vector<int64_t> nc(n), nd(n);
    {
        Phase ph("interval reduction (kernel, sync)");
        check(ctx, mth_lpmd_intervals_fetch(ctx, n, iv.tid.data(), iv.beg.data(), iv.end.data(), nc.data(), nd.data()));
    }
    if (g_shard.world > 1) { g_part->iv_c.swap(nc); g_part->iv_d.swap(nd); return; }
    intervals_write(nc, nd);
}

// ---- mhl-regions: MHL per interval of a BED file ---------------------------------------------------------------
// mhl (compute_mhl, mhl.rs:43-73, of the interval's own histograms), n_reads, max_cpgs.
// The rows are the sparse histograms (interval, length, runs, reads) sorted by (interval, length): one context's, or the shards' added.
void mhl_regions_write(const std::vector<uint32_t> &r_iv, const std::vector<uint32_t> &r_len, const std::vector<uint64_t> &r_runs,
                       const std::vector<uint64_t> &r_reads, uint32_t min_depth) {
    size_t o = 0;
    g_intervals.table(g_intervals.mhl_path, "mhl\tn_reads\tmax_cpgs", [&](LineWriter &w, size_t i) {
        const size_t o0 = o;
        while (o < r_iv.size() && r_iv[o] == (uint32_t)i) ++o;
        uint64_t n_reads = 0;
        uint32_t max_cpgs = 0;
        const float v = mth::mhl_regions_finalise(o - o0, r_len.data() + o0, r_runs.data() + o0, r_reads.data() + o0, min_depth, &n_reads, &max_cpgs);
        w.f32(v); w.ch('\t'); w.i64((long long)n_reads); w.ch('\t'); w.u32(max_cpgs);
    });
}

// the histograms counted on this context (a shard of several: its rows go to main(), which adds the shards' -- a read is owned by the
// shard that holds its start -- finalises once and writes the file)
void mhl_regions_finish(mth_ctx_t *ctx, uint32_t min_depth) {
    uint64_t k = 0;
    check(ctx, mth_mhl_regions_counts(ctx, &k, nullptr, nullptr, nullptr, nullptr));
    std::vector<uint32_t> r_iv(k), r_len(k);
    std::vector<uint64_t> r_runs(k), r_reads(k);
    check(ctx, mth_mhl_regions_counts(ctx, &k, r_iv.data(), r_len.data(), r_runs.data(), r_reads.data()));
    if (g_shard.world > 1) { g_part->mr_iv.swap(r_iv); g_part->mr_len.swap(r_len); g_part->mr_runs.swap(r_runs); g_part->mr_reads.swap(r_reads); return; }
    mhl_regions_write(r_iv, r_len, r_runs, r_reads, min_depth);
}

// ---- pdr-regions: PDR per interval of a BED file ---------------------------------------------------------------
// pdr (pdr.rs:47-49 of the interval's own counters), n_concordant, n_discordant, n_methylated.
// The three arrays are the contributing reads per class: one context's, or the shards' added.
void pdr_regions_write(const std::vector<uint64_t> &m, const std::vector<uint64_t> &u, const std::vector<uint64_t> &d, uint32_t min_depth) {
    g_intervals.table(g_intervals.pdr_path, "pdr\tn_concordant\tn_discordant\tn_methylated", [&](LineWriter &w, size_t i) {
        const uint64_t conc = m[i] + u[i];
        w.f32(mth::pdr_regions_finalise(conc, d[i], min_depth)); w.ch('\t'); w.i64((long long)conc); w.ch('\t'); w.i64((long long)d[i]); w.ch('\t');
        w.i64((long long)m[i]);
    });
}

// the counters of this context (a shard of several: its arrays go to main(), which adds the shards' -- a read is owned by the shard
// that holds its start -- finalises once and writes the file).  The first call that waits for the queued passes: their data errors
// surface here
void pdr_regions_finish(mth_ctx_t *ctx, uint32_t min_depth) {
    const size_t n = g_intervals.tid.size();
    std::vector<uint64_t> m(n), u(n), d(n);
    check(ctx, mth_pdr_regions_counts(ctx, m.data(), u.data(), d.data()));
    if (g_shard.world > 1) { g_part->pr_m.swap(m); g_part->pr_u.swap(u); g_part->pr_d.swap(d); return; }
    pdr_regions_write(m, u, d, min_depth);
}

// ---- me-regions / pm-regions: ME and PM per interval of a BED file ------------------------------------------------
// me (me.rs:42-55) or pm (pm.rs:42-51) of the interval's own pooled histogram, n_patterns, n_reads.
// bins: sixteen per interval, reads: one -- one context's, or the shards' added.  Either table, or both, from the same counters.
void quartet_regions_write(const std::vector<uint64_t> &bins, const std::vector<uint64_t> &reads, uint32_t min_depth) {
    for (const bool want_me : {true, false}) {
        const std::string &path = want_me ? g_intervals.me_path : g_intervals.pm_path;
        if (path.empty()) continue;
        g_intervals.table(path, want_me ? "me\tn_patterns\tn_reads" : "pm\tn_patterns\tn_reads", [&](LineWriter &w, size_t i) {
            float me = 0.0f, pm = 0.0f;
            uint64_t n_patterns = 0;
            mth::quartet_regions_finalise(bins.data() + i * 16, min_depth, &me, &pm, &n_patterns);
            w.f32(want_me ? me : pm); w.ch('\t'); w.i64((long long)n_patterns); w.ch('\t'); w.i64((long long)reads[i]);
        });
    }
}

// the counters of this context (a shard of several: its arrays go to main(), which adds the shards' -- a read is owned by the shard
// that holds its start -- finalises once and writes the file).  The first call that waits for the queued passes: their data errors
// surface here
void quartet_regions_finish(mth_ctx_t *ctx, uint32_t min_depth) {
    const size_t n = g_intervals.tid.size();
    std::vector<uint64_t> bins(n * 16), reads(n);
    check(ctx, mth_quartet_regions_counts(ctx, bins.data(), reads.data()));
    if (g_shard.world > 1) { g_part->qr_bins.swap(bins); g_part->qr_reads.swap(reads); return; }
    quartet_regions_write(bins, reads, min_depth);
}

// me.rs:68-88 / pm.rs:63-83: one line per quartet with depth >= min_depth,
// chrom, pos1..pos4, value (me.rs:57-65).  The reference iterates a HashMap (random order).
void quartet_write(mth_ctx_t *ctx, const Input &in, uint32_t min_depth, bool want_me, const std::string &path) {
    Phase ph("fetch + TSV write");
    uint64_t n = 0;
    check(ctx, mth_quartet_fetch(ctx, min_depth, &n, nullptr, nullptr, nullptr, nullptr, nullptr));
    std::vector<int32_t> tid(n), pos(n * 4);
    std::vector<float> val(n);
    check(ctx, mth_quartet_fetch(ctx, min_depth, &n, tid.data(), pos.data(), nullptr, want_me ? val.data() : nullptr,
                                 want_me ? nullptr : val.data()));
    FILE *f = open_output(path);
    write_rows(f, n, [&](LineWriter &w, uint64_t i) {
        w.str(mth_host_ref_name(in.h, tid[i]));
        for (int k = 0; k < 4; ++k) { w.ch('\t'); w.i32(pos[4 * i + k]); }
        w.ch('\t'); w.f32(val[i]); w.eol();
    });
    if (fclose(f) != 0) die("Error writing to output file.");
}

// mhl.rs:101-133: chrom, pos, pos+2, mhl -- sorted by (tid,pos)
void mhl_write(mth_ctx_t *ctx, const Input &in, const std::string &path) {
    uint64_t n = 0;
    check(ctx, mth_mhl_fetch(ctx, &n, nullptr, nullptr, nullptr, nullptr));
    std::vector<int32_t> tid(n), pos(n);
    std::vector<float> val(n);
    check(ctx, mth_mhl_fetch(ctx, &n, tid.data(), pos.data(), val.data(), nullptr));
    FILE *f = open_output(path);
    write_rows(f, n, [&](LineWriter &w, uint64_t i) {
        w.str(mth_host_ref_name(in.h, tid[i])); w.ch('\t'); w.i32(pos[i]); w.ch('\t'); w.i32(pos[i] + 2); w.ch('\t'); w.f32(val[i]); w.eol();
    });
    if (fclose(f) != 0) die("Error writing to output file.");
}

// fdrp.rs:148-174 / qfdrp.rs:160-186: chrom, pos, pos+2, value -- sorted by (tid,pos); either path may be empty
void fdrp_write(mth_ctx_t *ctx, const Input &in, const std::string &fdrp_path, const std::string &qfdrp_path) {
    uint64_t n = 0;
    check(ctx, mth_fdrp_fetch(ctx, &n, nullptr, nullptr, nullptr, nullptr, nullptr));
    std::vector<int32_t> tid(n), pos(n);
    std::vector<float> fv(fdrp_path.empty() ? 0 : n), qv(qfdrp_path.empty() ? 0 : n);
    check(ctx, mth_fdrp_fetch(ctx, &n, tid.data(), pos.data(), fdrp_path.empty() ? nullptr : fv.data(),
                              qfdrp_path.empty() ? nullptr : qv.data(), nullptr));
    for (int q = 0; q < 2; ++q) {
        const std::string &path = q ? qfdrp_path : fdrp_path;
        if (path.empty()) continue;
        const std::vector<float> &val = q ? qv : fv;
        FILE *f = open_output(path);
        write_rows(f, n, [&](LineWriter &w, uint64_t i) {
            w.str(mth_host_ref_name(in.h, tid[i])); w.ch('\t'); w.i32(pos[i]); w.ch('\t'); w.i32(pos[i] + 2); w.ch('\t'); w.f32(val[i]); w.eol();
        });
        if (fclose(f) != 0) die("Error writing to output file.");
    }
}

// ---- the single commands ----------------------------------------------------------------------------------------------------------

int run_pdr(const Args &a) {
    Input in = load(a.s.at("input"), a.has("cpg-set") ? a.s.at("cpg-set").c_str() : nullptr);
    mth_ctx_t *ctx = in.ctx ? in.ctx : make_ctx();
    mth_pdr_lpmd_params_t p;
    memset(&p, 0, sizeof p);
    p.pdr_min_depth = (uint32_t)a.n.at("min-depth");
    p.pdr_min_cpgs = (uint32_t)std::min<int64_t>(a.n.at("min-cpgs"), UINT32_MAX);
    p.pdr_min_qual = (uint8_t)a.n.at("min-qual");
    p.want_pdr = 1;
    if (in.file_order) {
        mth_fileorder_params_t fp;
        memset(&fp, 0, sizeof fp);
        fp.measure = MTH_FO_PDR; fp.min_depth = p.pdr_min_depth; fp.min_cpgs = p.pdr_min_cpgs; fp.min_qual = p.pdr_min_qual;
        return run_file_order(a, in, ctx, fp, 0);
    }
    {
        Phase ph("H2D + kernels (sync)");
        submit(ctx, in, p);
        uint64_t n = 0;
        check(ctx, mth_pdr_count(ctx, &n));
    }
    pdr_write(ctx, in, a.s.at("output"));
    return finish(ctx, in.h);
}

int run_lpmd(const Args &a) {
    const std::string input = a.s.at("input");
    const int32_t mind = (int32_t)a.n.at("min-distance"), maxd = (int32_t)a.n.at("max-distance");
    // lpmd.rs:161-164
    fprintf(stderr, "Computing subset-LPMD with parameters input=%s, min_distance=%d, max_distance=%d\n", input.c_str(), mind, maxd);
    g_shard.xm_min_mapq = (int)a.n.at("min-qual");      // lpmd.rs:176-181: the mapq filter comes before BismarkRead::new (the XM panic)
    g_shard.order_free = true;
    Input in = load(input, a.has("cpg-set") ? a.s.at("cpg-set").c_str() : nullptr);
    mth_ctx_t *ctx = in.ctx ? in.ctx : make_ctx();
    mth_pdr_lpmd_params_t p;
    memset(&p, 0, sizeof p);
    p.lpmd_min_qual = (uint8_t)a.n.at("min-qual");
    p.lpmd_min_distance = mind; p.lpmd_max_distance = maxd;
    p.want_lpmd = 1;
    submit(ctx, in, p);
    lpmd_write(ctx, in, input, p.lpmd_min_qual, a.s.at("output"));
    if (a.has("pairs") || g_intervals.on()) {                   // lpmd.rs:149-151, 89-122
        mth_lpmd_pairs_params_t pp;
        pp.min_distance = mind; pp.max_distance = maxd; pp.min_qual = p.lpmd_min_qual;
        for (const Contig &c : in.contigs) {
            const mth_batch_t b = make_batch(in, c);
            check(ctx, mth_lpmd_pairs_accumulate(ctx, &b, &pp));
        }
        if (a.has("pairs")) lpmd_pairs_write(ctx, in, a.s.at("pairs"));
        if (g_intervals.on()) lpmd_intervals_write(ctx);        // --intervals alone: the table stays on the device
    }
    return finish(ctx, in.h);
}

int run_quartet(const Args &a, bool want_me) {
    g_shard.order_free = true;
    Input in = load(a.s.at("input"), a.has("cpg-set") ? a.s.at("cpg-set").c_str() : nullptr);
    mth_ctx_t *ctx = in.ctx ? in.ctx : make_ctx();
    mth_quartet_params_t p;
    p.min_qual = (uint8_t)a.n.at("min-qual");
    {
        Phase ph("H2D + kernels (sync)");
        for (const Contig &c : in.contigs) {
            const mth_batch_t b = make_batch(in, c);
            check(ctx, mth_quartet_accumulate(ctx, &b, &p));
        }
    }
    quartet_write(ctx, in, (uint32_t)a.n.at("min-depth"), want_me, a.s.at("output"));
    return finish(ctx, in.h);
}

// -d / -p / -q of mhl and of the two per-interval measures
mth_mhl_params_t regions_params(const Args &a) {
    mth_mhl_params_t p;
    p.min_depth = (uint32_t)a.n.at("min-depth");
    p.min_cpgs = (uint32_t)std::min<int64_t>(a.n.at("min-cpgs"), UINT32_MAX);
    p.min_qual = (uint8_t)a.n.at("min-qual");
    return p;
}

int run_mhl(const Args &a) {
    Input in = load(a.s.at("input"), a.has("cpg-set") ? a.s.at("cpg-set").c_str() : nullptr);
    mth_ctx_t *ctx = in.ctx ? in.ctx : make_ctx();
    const mth_mhl_params_t p = regions_params(a);
    if (in.file_order) {
        mth_fileorder_params_t fp;
        memset(&fp, 0, sizeof fp);
        fp.measure = MTH_FO_MHL; fp.min_depth = p.min_depth; fp.min_cpgs = p.min_cpgs; fp.min_qual = p.min_qual;
        return run_file_order(a, in, ctx, fp, 1);
    }
    for (const Contig &c : in.contigs) {
        const mth_batch_t b = make_batch(in, c);
        check(ctx, mth_mhl_accumulate(ctx, &b, &p));
    }
    mhl_write(ctx, in, a.s.at("output"));
    return finish(ctx, in.h);
}

// mhl-regions / pdr-regions: every read counts once, whatever the order of the records, so input that is not coordinate-sorted is
// routed as lpmd routes it
int run_regions(const Args &a, bool pdr) {
    g_shard.order_free = true;
    Input in = load(a.s.at("input"), a.has("cpg-set") ? a.s.at("cpg-set").c_str() : nullptr);
    mth_ctx_t *ctx = in.ctx ? in.ctx : make_ctx();
    const mth_mhl_params_t p = regions_params(a);
    const Intervals &iv = g_intervals;
    {
        Phase ph("H2D + kernels (sync)");
        check(ctx, (pdr ? mth_pdr_regions_begin : mth_mhl_regions_begin)(ctx, iv.tid.size(), iv.tid.data(), iv.beg.data(), iv.end.data()));
        for (const Contig &c : in.contigs) {
            const mth_batch_t b = make_batch(in, c);
            check(ctx, (pdr ? mth_pdr_regions_accumulate : mth_mhl_regions_accumulate)(ctx, &b, &p));
        }
        if (pdr) check(ctx, mth_ctx_sync(ctx));           // (PDR's passes are queued: the phase's time is theirs only if it waits for them)
    }
    if (pdr) pdr_regions_finish(ctx, p.min_depth); else mhl_regions_finish(ctx, p.min_depth);
    return finish(ctx, in.h);
}

// me-regions / pm-regions: one function for both (the path main() has set says which table is written); order-free as the two above
int run_quartet_regions(const Args &a) {
    g_shard.order_free = true;
    Input in = load(a.s.at("input"), a.has("cpg-set") ? a.s.at("cpg-set").c_str() : nullptr);
    mth_ctx_t *ctx = in.ctx ? in.ctx : make_ctx();
    mth_quartet_params_t p;
    p.min_qual = (uint8_t)a.n.at("min-qual");
    const Intervals &iv = g_intervals;
    {
        Phase ph("H2D + kernels (sync)");
        check(ctx, mth_quartet_regions_begin(ctx, iv.tid.size(), iv.tid.data(), iv.beg.data(), iv.end.data()));
        for (const Contig &c : in.contigs) {
            const mth_batch_t b = make_batch(in, c);
            check(ctx, mth_quartet_regions_accumulate(ctx, &b, &p));
        }
        check(ctx, mth_ctx_sync(ctx));                        // (the passes are queued: the phase's time is theirs only if it waits for them)
    }
    quartet_regions_finish(ctx, (uint32_t)a.n.at("min-depth"));
    return finish(ctx, in.h);
}

int run_fdrp(const Args &a, bool quantitative) {
    Input in = load(a.s.at("input"), a.has("cpg-set") ? a.s.at("cpg-set").c_str() : nullptr);
    mth_ctx_t *ctx = in.ctx ? in.ctx : make_ctx();
    mth_fdrp_params_t p;
    memset(&p, 0, sizeof p);
    p.min_qual = (uint8_t)a.n.at("min-qual");
    p.min_depth = (uint64_t)a.n.at("min-depth");
    p.max_depth = (uint32_t)std::min<int64_t>(a.n.at("max-depth"), UINT32_MAX);
    p.min_overlap = (int32_t)a.n.at("min-overlap");
    const char *seed = getenv("METHEOR_SEED");       // reservoir draws (the reference's are OS-seeded)
    p.seed = seed ? strtoull(seed, nullptr, 10) : 0;
    if (in.file_order) {
        mth_fileorder_params_t fp;
        memset(&fp, 0, sizeof fp);
        fp.measure = MTH_FO_FDRP; fp.min_depth = (uint32_t)std::min<uint64_t>(p.min_depth, UINT32_MAX); fp.max_depth = p.max_depth;
        fp.min_overlap = p.min_overlap; fp.min_qual = p.min_qual; fp.seed = p.seed;
        return run_file_order(a, in, ctx, fp, quantitative ? 2 : 1);
    }
    for (const Contig &c : in.contigs) {
        const mth_batch_t b = make_batch(in, c);
        check(ctx, mth_fdrp_accumulate(ctx, &b, &p));
    }
    const std::string none;
    fdrp_write(ctx, in, quantitative ? none : a.s.at("output"), quantitative ? a.s.at("output") : none);
    return finish(ctx, in.h);
}

// ---- metheor all: any subset of the seven measures from ONE decode ----------------------------------------------------------------
// Each output file is byte for byte what the matching single command writes with the same parameters (`metheor pdr -i IN -o F -d ..
// -p .. -q ..` and so on).  What the single commands do differently on the way is taken care of here:
//   * the XM rule: lpmd alone decodes with its mapq-first rule (lpmd.rs:176-181), every other measure with the strict one -- `all` takes
//     the strict rule unless lpmd (and its pairs table) is all it was asked for: where that refuses a file, one of the requested single
//     runs refuses it too (exit 101);
//   * unsorted input: pdr / mhl / fdrp / qfdrp replay the decoded stream in file order (one replay per measure; FDRP's gives both
//     tables), then lpmd / me / pm sort the same decoded stream on the device (mth_decoded_sort) and take the batches -- or, where the
//     device sort cannot take the stream (records without a contig or an aligned base), a host decode of the file, as their single
//     runs do.
// On sorted input every batch (contig group) is accumulated once for all the requested measures (mth_multi_accumulate: one prepared
// batch, one read index).
int run_all(const Args &a) {
    const std::string input = a.s.at("input");
    const char *cpg_set = a.has("cpg-set") ? a.s.at("cpg-set").c_str() : nullptr;
    const bool w_pdr = a.has("pdr"), w_lpmd = a.has("lpmd"), w_pairs = a.has("lpmd-pairs"), w_iv = g_intervals.on(), w_mr = g_intervals.mhl_on(), w_pr = g_intervals.pdr_on(), w_qr = g_intervals.quartet_on(), w_mhl = a.has("mhl"), w_me = a.has("me"),
               w_pm = a.has("pm"), w_fdrp = a.has("fdrp"), w_qfdrp = a.has("qfdrp");
    const uint32_t min_depth = (uint32_t)a.n.at("min-depth");
    const uint32_t min_cpgs = (uint32_t)std::min<int64_t>(a.n.at("min-cpgs"), UINT32_MAX);
    const uint8_t min_qual = (uint8_t)a.n.at("min-qual");
    const int32_t mind = (int32_t)a.n.at("min-distance"), maxd = (int32_t)a.n.at("max-distance");
    if (w_lpmd)   // lpmd.rs:161-164
        fprintf(stderr, "Computing subset-LPMD with parameters input=%s, min_distance=%d, max_distance=%d\n", input.c_str(), mind, maxd);
    const bool any_flush = w_pdr || w_mhl || w_fdrp || w_qfdrp;          // the measures whose result depends on the record order
    const bool any_free = w_lpmd || w_me || w_pm || w_mr || w_pr || w_qr;
    g_shard.xm_min_mapq = (any_flush || w_me || w_pm || w_mr || w_pr || w_qr) ? 0 : (int)min_qual;
    g_shard.order_free = !any_flush;
    Input in = load(input, cpg_set);
    mth_ctx_t *ctx = in.ctx ? in.ctx : make_ctx();

    mth_multi_params_t mp;
    memset(&mp, 0, sizeof mp);
    mp.pdr_lpmd.pdr_min_depth = min_depth; mp.pdr_lpmd.pdr_min_cpgs = min_cpgs; mp.pdr_lpmd.pdr_min_qual = min_qual;
    mp.pdr_lpmd.lpmd_min_qual = min_qual; mp.pdr_lpmd.lpmd_min_distance = mind; mp.pdr_lpmd.lpmd_max_distance = maxd;
    mp.quartet.min_qual = min_qual;
    mp.mhl.min_depth = min_depth; mp.mhl.min_cpgs = min_cpgs; mp.mhl.min_qual = min_qual;
    mp.fdrp.min_qual = min_qual; mp.fdrp.min_depth = min_depth;
    mp.fdrp.max_depth = (uint32_t)std::min<int64_t>(a.n.at("max-depth"), UINT32_MAX);
    mp.fdrp.min_overlap = (int32_t)a.n.at("min-overlap");
    const char *seed = getenv("METHEOR_SEED");       // reservoir draws (the reference's are OS-seeded)
    mp.fdrp.seed = seed ? strtoull(seed, nullptr, 10) : 0;
    mp.pairs.min_distance = mind; mp.pairs.max_distance = maxd; mp.pairs.min_qual = min_qual;
    mp.form = MTH_MULTI_AUTO;
    const std::string none;

    Input host_in;                                   // (unsorted input the device sort cannot take: the order-free measures' host decode)
    Input *bin = &in;
    if (in.file_order) {
        mth_fileorder_params_t fp;
        memset(&fp, 0, sizeof fp);
        fp.min_qual = min_qual;
        if (w_pdr) {
            fp.measure = MTH_FO_PDR; fp.min_depth = min_depth; fp.min_cpgs = min_cpgs;
            file_order_write(in, ctx, fp, 0, a.s.at("pdr"));
        }
        if (w_mhl) {
            fp.measure = MTH_FO_MHL; fp.min_depth = min_depth; fp.min_cpgs = min_cpgs;
            file_order_write(in, ctx, fp, 1, a.s.at("mhl"));
        }
        if (w_fdrp || w_qfdrp) {
            fp.measure = MTH_FO_FDRP; fp.min_depth = min_depth; fp.min_cpgs = 0; fp.max_depth = mp.fdrp.max_depth;
            fp.min_overlap = mp.fdrp.min_overlap; fp.seed = mp.fdrp.seed;
            file_order_write(in, ctx, fp, 1, w_fdrp ? a.s.at("fdrp") : none, w_qfdrp ? &a.s.at("qfdrp") : nullptr);
        }
        if (!any_free) return finish(ctx, in.h);
        if (!(in.dec_flags & 3u)) {
            Phase ps("  device sort by (tid, start)");
            check(ctx, mth_decoded_sort(ctx));
            const uint32_t cap = (uint32_t)std::max(1, mth_host_n_refs(in.h)) + 1;
            std::vector<int32_t> tids(cap);
            std::vector<uint64_t> rb(cap), re(cap);
            uint32_t n_runs = 0, flags = 0;
            check(ctx, mth_decoded_contigs(ctx, cap, tids.data(), rb.data(), re.data(), &n_runs, &flags));
            in.file_order = false;
            if (!batch_decoded(in, tids, rb, re, n_runs, flags))
                die("metheor (MI355X path): the decoded stream could not be batched after the device sort");
        } else {
            g_shard.order_free = true;
            host_in = load(input, cpg_set, true, ctx);
            bin = &host_in;
        }
        mp.want = (w_lpmd ? MTH_MULTI_LPMD : 0u) | ((w_me || w_pm) ? MTH_MULTI_QUARTET : 0u) | ((w_pairs || w_iv) ? MTH_MULTI_PAIRS : 0u);
    } else {
        mp.want = (w_pdr ? MTH_MULTI_PDR : 0u) | (w_lpmd ? MTH_MULTI_LPMD : 0u) | ((w_me || w_pm) ? MTH_MULTI_QUARTET : 0u) |
                  (w_mhl ? MTH_MULTI_MHL : 0u) | ((w_fdrp || w_qfdrp) ? MTH_MULTI_FDRP : 0u) | ((w_pairs || w_iv) ? MTH_MULTI_PAIRS : 0u);
    }
    {
        Phase ph("H2D + kernels (sync)");
        const Intervals &iv = g_intervals;
        if (w_mr) check(ctx, mth_mhl_regions_begin(ctx, iv.tid.size(), iv.tid.data(), iv.beg.data(), iv.end.data()));
        if (w_pr) check(ctx, mth_pdr_regions_begin(ctx, iv.tid.size(), iv.tid.data(), iv.beg.data(), iv.end.data()));
        if (w_qr) check(ctx, mth_quartet_regions_begin(ctx, iv.tid.size(), iv.tid.data(), iv.beg.data(), iv.end.data()));
        for (const Contig &c : bin->contigs) {
            const mth_batch_t b = make_batch(*bin, c);
            mth_batch_t pb;
            check(ctx, mth_batch_prepare(ctx, &b, &pb));      // one device copy and one read index for every measure of the batch
            if (mp.want) check(ctx, mth_multi_accumulate(ctx, &pb, &mp));
            if (w_mr) check(ctx, mth_mhl_regions_accumulate(ctx, &pb, &mp.mhl));      // the per-interval MHL, on the batch as it is prepared
            if (w_pr) check(ctx, mth_pdr_regions_accumulate(ctx, &pb, &mp.mhl));      // ... and the per-interval PDR (queued; the release waits)
            if (w_qr) check(ctx, mth_quartet_regions_accumulate(ctx, &pb, &mp.quartet));      // ... and the per-interval ME / PM (queued as well)
            check(ctx, mth_batch_release(ctx, &pb));
        }
    }
    if (mp.want & MTH_MULTI_PDR) pdr_write(ctx, *bin, a.s.at("pdr"));
    if (w_lpmd) lpmd_write(ctx, *bin, input, min_qual, a.s.at("lpmd"));
    if (w_pairs) lpmd_pairs_write(ctx, *bin, a.s.at("lpmd-pairs"));
    if (w_iv) lpmd_intervals_write(ctx);
    if (w_mr) mhl_regions_finish(ctx, min_depth);
    if (w_pr) pdr_regions_finish(ctx, min_depth);
    if (w_qr) quartet_regions_finish(ctx, min_depth);
    if (w_me) quartet_write(ctx, *bin, min_depth, true, a.s.at("me"));
    if (w_pm) quartet_write(ctx, *bin, min_depth, false, a.s.at("pm"));
    if (mp.want & MTH_MULTI_MHL) mhl_write(ctx, *bin, a.s.at("mhl"));
    if (mp.want & MTH_MULTI_FDRP) fdrp_write(ctx, *bin, w_fdrp ? a.s.at("fdrp") : none, w_qfdrp ? a.s.at("qfdrp") : none);
    if (host_in.h) { mth_host_close(host_in.h); host_in.h = nullptr; }      // (the order-free measures' own decode of the file)
    return finish(ctx, in.h);
}

}  // namespace

// ---- metheor tag (src/tag.rs:386-443 run) ---------------------------------------------------------------------
// Same order of events as the reference: open the input (BAM or SAM text) and look at its first record's paired flag
// (bamutil.rs:27-37), refuse an output path whose parent is not a directory (tag.rs:396-403; a bare file name has the
// parent "" and is refused there too), create the output and write the header as it is (tag.rs:405-410), open the
// FASTA and fetch every @SQ contig (tag.rs:412-431, printing the two progress lines), then stream the records: the
// XM string of each is computed on the device (mth_tag_records), appended as the last optional field and the record is
// written as a SAM line (tag.rs:433-441).
struct TagState {
    mth_ctx_t *ctx = nullptr;
    mth_host_t *h = nullptr;
    FILE *out = nullptr;
    int paired = -1;
    std::string line, fail;
};
int tag_window(void *user, const uint8_t *buf, const uint64_t *rec_off, uint64_t n_rec) {
    TagState *st = static_cast<TagState *>(user);
    if (n_rec == 0) return 0;
    if (st->paired < 0) {                          // is_paired_end: the file's first record
        const uint64_t o = rec_off[0];
        st->paired = (rec_off[1] - o >= 36) ? ((buf[o + 4 + 14] | (buf[o + 4 + 15] << 8)) & 1) : 0;
    }
    mth_tag_out_t t{};
    const int rc = mth_tag_records(st->ctx, buf, rec_off[n_rec], rec_off, n_rec, MTH_MEM_HOST, st->paired, &t);
    if (rc != MTH_OK) {
        st->fail = std::string("metheor (MI355X path): ") + mth_strerror(rc) + (mth_last_error(st->ctx)[0] ? std::string(" -- ") + mth_last_error(st->ctx) : std::string());
        return 1;
    }
    std::vector<char> b;
    for (uint64_t i = 0; i < n_rec; ++i) {
        const uint8_t *rec = buf + rec_off[i] + 4;
        const uint32_t len = (uint32_t)(rec_off[i + 1] - rec_off[i] - 4);
        const int64_t cap = 4 * (int64_t)len + 256 + t.xm_len[i];
        if ((int64_t)b.size() < cap) b.resize((size_t)cap);
        int64_t n = mth_host_sam_format(st->h, rec, len, t.xm + t.xm_off[i], t.xm_len[i], b.data(), (int64_t)b.size());
        if (n > (int64_t)b.size()) {      // B:c / B:s arrays print up to 7 characters per 1-2 byte element: the formatter says how much it needs
            b.resize((size_t)n);
            n = mth_host_sam_format(st->h, rec, len, t.xm + t.xm_off[i], t.xm_len[i], b.data(), (int64_t)b.size());
        }
        if (n < 0 || n > (int64_t)b.size()) { st->fail = "metheor: cannot format a record as SAM (malformed BAM record)"; return 1; }
        if (fwrite(b.data(), 1, (size_t)n, st->out) != (size_t)n) { st->fail = "Error writing to output file."; return 1; }
    }
    return 0;
}

// --output-format bam: the window's tagged records come back as finished BGZF blocks (mth_tag_records_bam: record stream,
// block cuts by htslib's rule and DEFLATE on the device) and go to the file as they are
int tag_window_bam(void *user, const uint8_t *buf, const uint64_t *rec_off, uint64_t n_rec) {
    TagState *st = static_cast<TagState *>(user);
    if (n_rec == 0) return 0;
    if (st->paired < 0) {                          // is_paired_end: the file's first record
        const uint64_t o = rec_off[0];
        st->paired = (rec_off[1] - o >= 36) ? ((buf[o + 4 + 14] | (buf[o + 4 + 15] << 8)) & 1) : 0;
    }
    mth_tag_bam_out_t t{};
    const int rc = mth_tag_records_bam(st->ctx, buf, rec_off[n_rec], rec_off, n_rec, MTH_MEM_HOST, st->paired, &t);
    if (rc != MTH_OK) {
        st->fail = std::string("metheor (MI355X path): ") + mth_strerror(rc) + (mth_last_error(st->ctx)[0] ? std::string(" -- ") + mth_last_error(st->ctx) : std::string());
        return 1;
    }
    if (t.n_bytes && fwrite(t.bytes, 1, (size_t)t.n_bytes, st->out) != (size_t)t.n_bytes) { st->fail = "Error writing to output file."; return 1; }
    return 0;
}

// n bytes as BGZF blocks of at most 0xff00 bytes each, compressed on the host (the BAM header: a few blocks at most)
bool bgzf_write_host(FILE *out, const uint8_t *p, size_t n) {
    std::vector<uint8_t> blk(18 + compressBound(0xff00) + 8);
    for (size_t i = 0; i < n;) {
        const size_t k = std::min<size_t>(n - i, 0xff00);
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (deflateInit2(&zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
        zs.next_in = const_cast<uint8_t *>(p + i); zs.avail_in = (uInt)k;
        zs.next_out = blk.data() + 18; zs.avail_out = (uInt)(blk.size() - 26);
        const int zr = deflate(&zs, Z_FINISH);
        const size_t clen = blk.size() - 26 - zs.avail_out;
        deflateEnd(&zs);
        if (zr != Z_STREAM_END || 18 + clen + 8 > 65536) return false;
        const uint8_t hdr[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0};
        memcpy(blk.data(), hdr, 16);
        const uint32_t bsize = (uint32_t)(clen + 25), crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), p + i, (uInt)k), isize = (uint32_t)k;
        blk[16] = (uint8_t)bsize; blk[17] = (uint8_t)(bsize >> 8);
        for (int b = 0; b < 4; ++b) { blk[18 + clen + b] = (uint8_t)(crc >> (8 * b)); blk[22 + clen + b] = (uint8_t)(isize >> (8 * b)); }
        if (fwrite(blk.data(), 1, 26 + clen, out) != 26 + clen) return false;
        i += k;
    }
    return true;
}

int run_tag(const Args &a) {
    const std::string input = a.s.at("input"), output = a.s.at("output"), genome = a.s.at("genome");
    const bool as_bam = a.has("output-format") && a.s.at("output-format") == "bam";
    const bool write_index = as_bam && a.has("write-index");
    const std::string index_path = output + ".bai";             // the first name mth_host_plan_region looks for
    CtxFuture cf;
    cf.start();
    mth_host_t *h = nullptr;
    char err[1024];
    if (mth_host_open(input.c_str(), &h, err, sizeof err) != 0) { cf.wait(); die(err); }   // bamutil.rs:4-11
    // tag.rs:396-403: PathBuf::from(output).parent() must be a directory
    {
        const size_t slash = output.rfind('/');
        const std::string dir = slash == std::string::npos ? std::string() : (slash == 0 ? std::string("/") : output.substr(0, slash));
        struct stat sb;
        if (dir.empty() || stat(dir.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode)) { cf.wait(); die("No such directory for output alignment file: " + dir); }
    }
    FILE *out = fopen(output.c_str(), "wb");
    if (!out) { cf.wait(); die("Error opening alignment file to write: " + output + ": " + strerror(errno)); }
    static char obuf[1 << 20];
    setvbuf(out, obuf, _IOFBF, sizeof obuf);
    // an index left over from another file of this name must not outlive it, whatever becomes of this run
    if (write_index && remove(index_path.c_str()) != 0 && errno != ENOENT) { cf.wait(); die("Error removing the old BAM index: " + index_path + ": " + strerror(errno)); }
    long header_bytes = 0;
    {   // the header text as it is, newline-terminated (Header::from_template strips and re-adds the final newline)
        uint64_t n = 0;
        const char *t = mth_host_header_text(h, &n);
        std::string text(t, strnlen(t, (size_t)n));
        while (!text.empty() && text.back() == '\n') text.pop_back();
        if (!text.empty()) text += '\n';
        if (!as_bam) {
            if (!text.empty()) fwrite(text.data(), 1, text.size(), out);
        } else {
            // the BAM header in BGZF blocks of its own: magic, l_text + the same text, n_ref + the names and lengths
            std::vector<uint8_t> hb;
            auto put32 = [&](uint32_t x) { for (int i = 0; i < 4; ++i) hb.push_back((uint8_t)(x >> (8 * i))); };
            hb.insert(hb.end(), {'B', 'A', 'M', 1});
            put32((uint32_t)text.size());
            hb.insert(hb.end(), text.begin(), text.end());
            const int n_ref = mth_host_n_refs(h);
            put32((uint32_t)n_ref);
            for (int t2 = 0; t2 < n_ref; ++t2) {
                const char *name = mth_host_ref_name(h, t2);
                const size_t ln = strlen(name) + 1;
                put32((uint32_t)ln);
                hb.insert(hb.end(), name, name + ln);
                put32((uint32_t)mth_host_ref_len(h, t2));
            }
            if (!bgzf_write_host(out, hb.data(), hb.size())) { cf.wait(); fflush(out); die("Error writing to output file."); }
            header_bytes = ftell(out);                          // where the first block of records will lie
        }
    }
    mth_fasta_t *fa = genome_open(genome, [&] { cf.wait(); fflush(out); });
    printf("Parsing reference genome...\n");
    mth_ctx_t *ctx = cf.get();
    {
        Phase ph("genome -> device");
        Genome g;
        if (genome_wants_device(fa)) genome_layout(fa, h, g, [&] { fflush(out); });
        else genome_fetch(fa, h, g, [&] { fflush(out); });
        genome_upload(ctx, h, g, [&] { fflush(out); });
    }
    printf("Done!\n");
    fflush(stdout);
    TagState st;
    st.ctx = ctx; st.h = h; st.out = out;
    if (!as_bam) {
        Phase ph("records -> XM -> SAM");
        const int rc = mth_host_decode_stream(h, tag_window, &st);
        if (rc != 0) { fflush(out); die(!st.fail.empty() ? st.fail : std::string("Error reading BAM record. ") + mth_host_last_error(h)); }
    } else {
        const bool timing = getenv("METHEOR_TIMING") != nullptr;
        if (timing) { mth_timing_reset(ctx); mth_timing_enable(ctx, 1); }
        if (write_index) {
            if (header_bytes < 0) { fflush(out); die("Error writing to output file."); }
            const int n_ref = mth_host_n_refs(h);
            std::vector<int64_t> ln((size_t)std::max(n_ref, 0));
            for (int t2 = 0; t2 < n_ref; ++t2) ln[(size_t)t2] = mth_host_ref_len(h, t2);
            if (mth_bai_begin(ctx, n_ref, ln.data(), (uint64_t)header_bytes) != MTH_OK) { fflush(out); die(std::string("metheor (MI355X path): ") + mth_last_error(ctx)); }
        }
        {
            Phase ph("records -> XM -> BAM");
            const int rc = mth_host_decode_stream(h, tag_window_bam, &st);
            if (rc != 0) { fflush(out); die(!st.fail.empty() ? st.fail : std::string("Error reading BAM record. ") + mth_host_last_error(h)); }
        }
        auto print_timing = [&] {
            if (!timing) return;
            for (const char *k : {"k_tag_assemble", "k_crc32", "k_deflate", "k_bgzf_compact", "bgzf_d2h", "k_bai_keys", "k_bai_rows", "bai_sort", "k_bai_fill"}) {
                double ms = 0;
                uint64_t n = 0;
                if (mth_timing_get(ctx, k, &ms, &n) == MTH_OK && n) fprintf(stderr, "[metheor timing]     tag/%-14s %.3f ms in %llu launches\n", k, ms * (double)n, (unsigned long long)n);
            }
            mth_timing_enable(ctx, 0);
        };
        if (!write_index) print_timing();
        static const uint8_t eof_block[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const long eof_off = write_index ? ftell(out) : 0;
        if (eof_off < 0 || fwrite(eof_block, 1, sizeof eof_block, out) != sizeof eof_block) die("Error writing to output file.");
        if (fclose(out) != 0) die("Error writing to output file.");
        out = nullptr;
        if (write_index) {
            // the BAM is complete; the index follows in one piece, or not at all.  The EOF block is an empty block behind the last
            // record: the library gives that record the block's offset as its end, as bgzf_tell reports it there
            Phase ph("index -> .bai");
            const uint64_t cut[2] = {0, 0}, coff[1] = {(uint64_t)eof_off};
            mth_bai_out_t ix{};
            int rc = mth_bai_add_records(ctx, nullptr, nullptr, 0, MTH_MEM_HOST, cut, coff, 1);
            if (rc == MTH_OK) rc = mth_bai_finish(ctx, &ix);
            print_timing();
            if (rc != MTH_OK) die("metheor: " + output + " is complete, but no index is written: " + mth_last_error(ctx));
            mth_host_bai_tables_t tb{};
            tb.n_refs = ix.n_refs; tb.n_chunks = ix.n_chunks; tb.chunk_beg = ix.chunk_beg; tb.chunk_end = ix.chunk_end; tb.n_bins = ix.n_bins;
            tb.bin_ref = ix.bin_ref; tb.bin_id = ix.bin_id; tb.bin_n_chunks = ix.bin_n_chunks; tb.ref_n_bins = ix.ref_n_bins; tb.ref_n_intv = ix.ref_n_intv;
            tb.lin_off = ix.lin_off; tb.lin = ix.lin; tb.meta = ix.meta; tb.n_no_coor = ix.n_no_coor;
            if (mth_host_bai_write(index_path.c_str(), &tb, err, sizeof err) != MTH_HOST_OK) die(err);
            if (timing) fprintf(stderr, "[metheor timing]     tag/index: %llu chunks in %llu bins\n", (unsigned long long)ix.n_chunks, (unsigned long long)ix.n_bins);
        }
    }
    if (out && fclose(out) != 0) die("Error writing to output file.");
    mth_host_fasta_close(fa);
    return finish(ctx, h);
}

int main(int argc, char **argv) {
    if (argc < 2) { print_main_help(stderr); return 2; }   // arg_required_else_help (lib.rs:18)
    const std::string sub = argv[1];
    if (sub == "-h" || sub == "--help" || sub == "help") { print_main_help(stdout); return 0; }
    if (sub == "-V" || sub == "--version") { printf("metheor 0.1.9\n"); return 0; }
    const Cmd *cmd = nullptr;
    for (const Cmd &c : commands()) if (sub == c.name) cmd = &c;
    if (!cmd) {
        if (!sub.empty() && sub[0] == '-') usage_error(nullptr, "unexpected argument '" + sub + "' found");
        usage_error(nullptr, "unrecognized subcommand '" + sub + "'");
    }
    const Args a = parse_args(*cmd, argc, argv, 2);
    // HIP runtime setting for a process that keeps one or two streams busy per device (read by the runtime at its first call; a value
    // from the caller's environment wins): one hardware queue per device shortens the load phase by ~25 ms on the 10 M-read file
    // (profiles/r02_e2e.md, "Runtime settings"; HIP_FORCE_DEV_KERNARG, HSA_ENABLE_INTERRUPT=0, HSA_ENABLE_SDMA=0 and others: no gain)
    setenv("GPU_MAX_HW_QUEUES", "1", 0);
    auto run = [&]() -> int {
        if (sub == "pdr") return run_pdr(a);
        if (sub == "lpmd") return run_lpmd(a);
        if (sub == "mhl") return run_mhl(a);
        if (sub == "mhl-regions") return run_regions(a, false);
        if (sub == "pdr-regions") return run_regions(a, true);
        if (sub == "me-regions" || sub == "pm-regions") return run_quartet_regions(a);
        if (sub == "fdrp") return run_fdrp(a, false);
        if (sub == "qfdrp") return run_fdrp(a, true);
        if (sub == "me") return run_quartet(a, true);
        if (sub == "pm") return run_quartet(a, false);
        if (sub == "all") return run_all(a);
        return -1;
    };
    if (sub == "tag") {
        if (a.has("output-format") && a.s.at("output-format") != "sam" && a.s.at("output-format") != "bam")
            usage_error(cmd, "invalid value '" + a.s.at("output-format") + "' for '--output-format <OUTPUT_FORMAT>'\n  [possible values: sam, bam]");
        if (a.has("write-index") && !(a.has("output-format") && a.s.at("output-format") == "bam"))
            usage_error(cmd, "the argument '--write-index' cannot be used without '--output-format bam'");
        if (const char *dev = getenv("METHEOR_DEVICE")) g_shard.device = atoi(dev);
        return run_tag(a);
    }
    if (sub == "all") {      // clap-style: an ArgGroup of the outputs (required, multiple) and `requires` on --lpmd-pairs
        static const char *outs[] = {"pdr", "lpmd", "mhl", "me", "pm", "fdrp", "qfdrp", "mhl-intervals", "pdr-intervals", "me-intervals", "pm-intervals"};
        bool any = false;
        for (const char *o : outs) any |= a.has(o);
        if (!any)
            usage_error(cmd, "the following required arguments were not provided:\n  <--pdr <PDR>|--lpmd <LPMD>|--mhl <MHL>|--me <ME>|--pm <PM>|--fdrp <FDRP>|--qfdrp <QFDRP>|--mhl-intervals <MHL_INTERVALS>|--pdr-intervals <PDR_INTERVALS>|--me-intervals <ME_INTERVALS>|--pm-intervals <PM_INTERVALS>>");
        if (a.has("lpmd-pairs") && !a.has("lpmd")) usage_error(cmd, "the following required arguments were not provided:\n  --lpmd <LPMD>");
        // the BED comes with at least one of its tables and each table with the BED; the LPMD table is LPMD's, the MHL, the PDR, the ME and
        // the PM table stand alone
        const bool own_table = a.has("mhl-intervals") || a.has("pdr-intervals") || a.has("me-intervals") || a.has("pm-intervals");
        if (a.has("intervals") && !a.has("lpmd-intervals") && !own_table)
            usage_error(cmd, "the following required arguments were not provided:\n  <--lpmd-intervals <LPMD_INTERVALS>|--mhl-intervals <MHL_INTERVALS>|--pdr-intervals <PDR_INTERVALS>|--me-intervals <ME_INTERVALS>|--pm-intervals <PM_INTERVALS>>");
        if ((a.has("lpmd-intervals") || own_table) && !a.has("intervals")) usage_error(cmd, "the following required arguments were not provided:\n  --intervals <INTERVALS>");
        if (a.has("lpmd-intervals") && !a.has("lpmd")) usage_error(cmd, "the following required arguments were not provided:\n  --lpmd <LPMD>");
        // a region owns reads by their start: an interval at its left edge would see part of its reads
        if (a.has("mhl-intervals") && a.has("region")) usage_error(cmd, "the argument '--mhl-intervals <MHL_INTERVALS>' cannot be used with '--region <REGION>'");
        if (a.has("pdr-intervals") && a.has("region")) usage_error(cmd, "the argument '--pdr-intervals <PDR_INTERVALS>' cannot be used with '--region <REGION>'");
        if (a.has("me-intervals") && a.has("region")) usage_error(cmd, "the argument '--me-intervals <ME_INTERVALS>' cannot be used with '--region <REGION>'");
        if (a.has("pm-intervals") && a.has("region")) usage_error(cmd, "the argument '--pm-intervals <PM_INTERVALS>' cannot be used with '--region <REGION>'");
    }
    if (sub == "lpmd") {     // `requires`, both ways
        if (a.has("intervals") && !a.has("intervals-output")) usage_error(cmd, "the following required arguments were not provided:\n  --intervals-output <INTERVALS_OUTPUT>");
        if (a.has("intervals-output") && !a.has("intervals")) usage_error(cmd, "the following required arguments were not provided:\n  --intervals <INTERVALS>");
    }
    if (a.has("genome")) g_genome.path = a.s.at("genome");
    if (a.has("mm-threshold") && !a.has("mm-tags")) usage_error(cmd, "the argument '--mm-threshold <MM_THRESHOLD>' cannot be used without '--mm-tags'");
    if (a.has("mm-tags") && a.has("genome")) usage_error(cmd, "the argument '--mm-tags' cannot be used with '--genome <GENOME>'");
    if (a.has("mm-tags")) { g_modtags = true; g_mm_threshold = (uint32_t)a.n.at("mm-threshold"); }
    // (`all` has no --gpus: one device)
    const int64_t gpus = a.n.count("gpus") ? a.n.at("gpus") : 1;
    int64_t halo = 65536;
    if (const char *e = getenv("METHEOR_SHARD_HALO")) { const long long k = atoll(e); if (k >= 0) halo = k; }
    if (a.has("region")) {       // chr | chr:beg-end (1-based, inclusive, commas allowed; as samtools view takes it)
        const std::string reg = a.s.at("region");
        g_shard.region = true; g_shard.region_name = reg;
        const size_t c = reg.rfind(':');
        if (c != std::string::npos && c + 1 < reg.size()) {
            std::string t;
            for (char ch : reg.substr(c + 1)) if (ch != ',') t.push_back(ch);
            long long b = 0, e = 0;
            char tail = 0;
            const int k = sscanf(t.c_str(), "%lld-%lld%c", &b, &e, &tail);
            if (k == 2 && b >= 1 && e >= b && e <= INT32_MAX) { g_shard.region_name = reg.substr(0, c); g_shard.r_beg = (int32_t)(b - 1); g_shard.r_end = (int32_t)e; }
            else if (k == 2 || reg.find('-', c) != std::string::npos) usage_error(cmd, "invalid value '" + reg + "' for '--region <REGION>': want chr or chr:beg-end with 1 <= beg <= end");
        }
        if (a.has("bai")) g_shard.bai = a.s.at("bai");
        if (gpus > 1) usage_error(cmd, "the argument '--region <REGION>' cannot be used with '--gpus <GPUS>' above 1");
    } else if (a.has("bai")) usage_error(cmd, "the argument '--bai <BAI>' needs '--region <REGION>'");
    const int world = (int)std::min<int64_t>(gpus, 4096);
    if (world < 1) usage_error(cmd, "invalid value '0' for '--gpus <GPUS>': at least one GPU");
    if (a.has("intervals")) {    // the BED is read against the input's header before any device or output file is touched
        g_intervals.path = a.s.at("intervals");
        if (sub == "mhl-regions") g_intervals.mhl_path = a.s.at("output");
        else if (sub == "pdr-regions") g_intervals.pdr_path = a.s.at("output");
        else if (sub == "me-regions") g_intervals.me_path = a.s.at("output");
        else if (sub == "pm-regions") g_intervals.pm_path = a.s.at("output");
        else if (sub == "lpmd") g_intervals.out_path = a.s.at("intervals-output");
        else {
            if (a.has("lpmd-intervals")) g_intervals.out_path = a.s.at("lpmd-intervals");
            if (a.has("mhl-intervals")) g_intervals.mhl_path = a.s.at("mhl-intervals");
            if (a.has("pdr-intervals")) g_intervals.pdr_path = a.s.at("pdr-intervals");
            if (a.has("me-intervals")) g_intervals.me_path = a.s.at("me-intervals");
            if (a.has("pm-intervals")) g_intervals.pm_path = a.s.at("pm-intervals");
        }
        mth_host_t *h = nullptr;
        char err[1024];
        if (mth_host_open(a.s.at("input").c_str(), &h, err, sizeof err) != 0) die(err);
        { Phase ph("intervals BED (header + parse)"); intervals_read(h); }
        mth_host_close(h);
    }
    if (world == 1) {
        if (const char *dev = getenv("METHEOR_DEVICE")) g_shard.device = atoi(dev);
        g_shard.halo = halo;
        return run();
    }
    // --gpus N: shard r runs on its own thread with its own context on device r mod the devices in use
    int ndev = 0;
    mth_device_count(&ndev);
    if (const char *e = getenv("METHEOR_DEVICES")) { const int k = atoi(e); if (k >= 1 && k < ndev) ndev = k; }
    if (ndev < 1) die(std::string("metheor (MI355X path): ") + mth_strerror(MTH_ERR_NO_DEVICE));
    {   // the reference opens the BAM before anything else: report an unreadable input once, not once per shard
        mth_host_t *h = nullptr;
        char err[1024];
        if (mth_host_open(a.s.at("input").c_str(), &h, err, sizeof err) != 0) die(err);
        genome_read_once(h, [] {});          // one host copy of the genome for all the shards
        mth_host_close(h);
    }
    std::vector<Part> parts((size_t)world);
    std::vector<std::thread> th;
    g_threads.store(true);
    for (int r = 0; r < world; ++r)
        th.emplace_back([&, r] {
            g_shard.rank = r; g_shard.world = world; g_shard.device = r % ndev; g_shard.halo = halo;
            g_part = &parts[(size_t)r];
            run();
        });
    for (auto &t : th) t.join();
    auto write_parts = [&](const std::string &path, bool pairs) {
        FILE *f = open_file(path);
        for (const Part &p : parts) {
            const char *b = pairs ? p.pairs : p.out;
            const size_t n = pairs ? p.pairs_len : p.out_len;
            if (n && fwrite(b, 1, n, f) != n) die("Error writing to output file.");
        }
        if (fclose(f) != 0) die("Error writing to output file.");
    };
    if (sub != "mhl-regions" && sub != "pdr-regions" && sub != "me-regions" && sub != "pm-regions") write_parts(a.s.at("output"), false);
    if (sub == "lpmd" && a.has("pairs")) write_parts(a.s.at("pairs"), true);
    if (g_intervals.mhl_on()) {  // every shard counted its own reads for all the intervals: the histograms add up, the value is finalised once
        std::map<std::pair<uint32_t, uint32_t>, std::pair<uint64_t, uint64_t>> sum;
        for (const Part &p : parts)
            for (size_t i = 0; i < p.mr_iv.size(); ++i) {
                auto &e = sum[{p.mr_iv[i], p.mr_len[i]}];
                e.first += p.mr_runs[i]; e.second += p.mr_reads[i];
            }
        std::vector<uint32_t> r_iv, r_len;
        std::vector<uint64_t> r_runs, r_reads;
        for (const auto &kv : sum) { r_iv.push_back(kv.first.first); r_len.push_back(kv.first.second); r_runs.push_back(kv.second.first); r_reads.push_back(kv.second.second); }
        mhl_regions_write(r_iv, r_len, r_runs, r_reads, (uint32_t)a.n.at("min-depth"));
    }
    if (g_intervals.pdr_on()) {  // ... and so do the three counters of the per-interval PDR
        const size_t n = g_intervals.tid.size();
        std::vector<uint64_t> m(n, 0), u(n, 0), d(n, 0);
        for (const Part &p : parts)
            for (size_t i = 0; i < n && i < p.pr_m.size(); ++i) { m[i] += p.pr_m[i]; u[i] += p.pr_u[i]; d[i] += p.pr_d[i]; }
        pdr_regions_write(m, u, d, (uint32_t)a.n.at("min-depth"));
    }
    if (g_intervals.quartet_on()) {  // ... and the seventeen of the per-interval ME / PM
        const size_t n = g_intervals.tid.size();
        std::vector<uint64_t> bins(n * 16, 0), reads(n, 0);
        for (const Part &p : parts) {
            for (size_t i = 0; i < bins.size() && i < p.qr_bins.size(); ++i) bins[i] += p.qr_bins[i];
            for (size_t i = 0; i < n && i < p.qr_reads.size(); ++i) reads[i] += p.qr_reads[i];
        }
        quartet_regions_write(bins, reads, (uint32_t)a.n.at("min-depth"));
    }
    if (g_intervals.on()) {      // every shard reduced its own rows for all the intervals: the sums add up
        const size_t n = g_intervals.tid.size();
        std::vector<int64_t> nc(n, 0), nd(n, 0);
        for (const Part &p : parts)
            for (size_t i = 0; i < n && i < p.iv_c.size(); ++i) { nc[i] += p.iv_c[i]; nd[i] += p.iv_d[i]; }
        intervals_write(nc, nd);
    }
    fflush(nullptr);
    _exit(0);
}
