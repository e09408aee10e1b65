// mecat2cns — drop-in for the reference's mecat2cns (src/mecat2cns/main.cpp, options.cpp, reads_correction_can.cpp,
// reads_correction_m4.cpp) on top of the C ABI: the same command line, the same partition and index files beside the input, the same
// output text.  Per partition file the reference's order of records (std::sort over the whole array by sid alone,
// reads_correction_aux.cpp:102), its two gates in front of a template (reads_correction_can.cpp:32-33) and one
// mhip_cns_correct_templates call whose FASTA text is appended to the output.
//
// Where this program differs from the reference:
//   - `-x` as the last word: the reference reads argv[argc] (options.cpp:168-173); here its message, the usage text, exit 1.
//   - an invalid `-x` argument: the reference prints an options struct it never filled in; here the options block is left out.
//   - letters other than A, C, G, T: stored as A (the reference draws rand() & 3, packed_db.cpp:158).
//   - the output is in template order within a partition, whatever -t is: what the reference writes with -t 1 (its multi-threaded
//     order is a race).  -t sizes the host thread pools only.
//   - -k is read, checked and printed; the partition files' bytes do not depend on it (host/partition.h).
//   - the whole read set is ONE volume: a set that does not fit, or a read of MAX_SEQ_SIZE letters or more, is refused with a message.
// MECAT_CNS_HOST_TEXT=1: the records and letters are copied to the host and formatted there (mhip_cns_format_reads) instead of on the
// device — the same bytes; for the A/B measurement (tools/cns_cli_time.py) and a test.
#include <getopt.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>
#include <unistd.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../host/partition.h"
#include "../host/volume.h"
#include "cns_groups.h"
#include "mecat_hip.h"

namespace {

const long kMaxSeqSize = 500000;      // MAX_SEQ_SIZE, common/defs.h:202

struct Options {
    int input_type = 1;               // options.cpp:10: m4 is the default
    const char *input = nullptr, *reads = nullptr, *output = nullptr;
    int num_threads = 1;
    long long batch_size = 100000;
    double min_mapping_ratio = 0.9;
    int min_align_size = 2000, min_cov = 6;
    long long min_size = 5000;
    bool usage = false;
    int tech = 0, num_partition_files = 10;
};

Options defaults_of(int tech) {
    Options o;
    o.tech = tech;
    if (tech == 1) { o.min_mapping_ratio = 0.4; o.min_align_size = 400; o.min_size = 2000; }
    return o;
}

void print_default_line(const Options& o) {
    fprintf(stderr, "-i %d -t %d -p %lld -r %g -a %d -c %d -l %lld -k %d\n", o.input_type, o.num_threads, o.batch_size, o.min_mapping_ratio, o.min_align_size, o.min_cov, o.min_size,
            o.num_partition_files);
}

void print_usage(const char* prog) {
    fprintf(stderr, "USAGE:\n%s [options] input reads output\n", prog);
    fprintf(stderr, "\nOPTIONS:\n");
    fprintf(stderr, "-x <0/1>\tsequencing platform: 0 = PACBIO, 1 = NANOPORE\n\t\tdefault: 0\n");
    fprintf(stderr, "-i <0/1>\tinput type: 0 = candidte, 1 = m4\n");
    fprintf(stderr, "-t <Integer>\tnumber of threads (CPUs)\n");
    fprintf(stderr, "-p <Integer>\tbatch size that the reads will be partitioned\n");
    fprintf(stderr, "-r <Real>\tminimum mapping ratio\n");
    fprintf(stderr, "-a <Integer>\tminimum overlap size\n");
    fprintf(stderr, "-c <Integer>\tminimum coverage under consideration\n");
    fprintf(stderr, "-l <Integer>\tminimum length of corrected sequence\n");
    fprintf(stderr, "-k <Integer>\tnumber of partition files when partitioning overlap results (if < 0, then it will be set to system limit value)\n");
    fprintf(stderr, "-h\t\tprint usage info.\n");
    fprintf(stderr, "\nIf 'x' is set to be '0' (pacbio), then the other options have the following default values: \n");
    print_default_line(defaults_of(0));
    fprintf(stderr, "\nIf 'x' is set to be '1' (nanopore), then the other options have the following default values: \n");
    print_default_line(defaults_of(1));
}

// the reference's labels as they are: the three file names stand under the wrong ones (options.cpp:292-294)
void print_options(const Options& o) {
    printf("input_type:\t%d\n", o.input_type);
    if (o.input) printf("reads\t%s\n", o.input);
    if (o.reads) printf("output\t%s\n", o.reads);
    if (o.output) printf("m4\t%s\n", o.output);
    printf("number of threads:\t%d\n", o.num_threads);
    printf("batch size:\t%lld\n", o.batch_size);
    printf("mapping ratio:\t%g\n", o.min_mapping_ratio);
    printf("align size:\t%d\n", o.min_align_size);
    printf("cov:\t%d\n", o.min_cov);
    printf("min size:\t%lld\n", o.min_size);
    printf("partition files:\t%d\n", o.num_partition_files);
    printf("tech:\t%d\n", o.tech);
}

// the technology picks the defaults, so it is looked for before the options are read (detect_tech, options.cpp:161-186).
// -> 0 / 1; -1: refused (message printed); -2: `-x` is the last word (message printed)
int detect_tech(int argc, char** argv) {
    for (int i = 0; i < argc; ++i) {
        if (strcmp(argv[i], "-x") != 0) continue;
        if (i + 1 == argc) { fprintf(stderr, "argument to option 'x' is missing.\n"); return -2; }
        printf("-x\n");
        if (argv[i + 1][0] == '0') return 0;
        if (argv[i + 1][0] == '1') return 1;
        fprintf(stderr, "invalid argument to option 'x': %s\n", argv[i + 1]);
        return -1;
    }
    return 0;
}

// 0: go on; 1: refused.  *filled: the options hold defaults and what was read so far (the reference prints them either way)
int parse_arguments(int argc, char** argv, Options& o, bool* filled) {
    *filled = false;
    const int tech = detect_tech(argc, argv);
    if (tech < 0) return 1;
    o = defaults_of(tech);
    *filled = true;
    opterr = 0;
    int ch;
    while ((ch = getopt(argc, argv, "i:t:p:r:a:c:l:x:k:h")) != -1) {
        switch (ch) {
            case 'i':
                if (optarg[0] == '0') o.input_type = 0;
                else if (optarg[0] == '1') o.input_type = 1;
                else { fprintf(stderr, "invalid argument to option 'i': %s\n", optarg); return 1; }
                break;
            case 't': o.num_threads = atoi(optarg); break;
            case 'p': o.batch_size = atoll(optarg); break;
            case 'r': o.min_mapping_ratio = atof(optarg); break;
            case 'a': o.min_align_size = atoi(optarg); break;
            case 'c': o.min_cov = atoi(optarg); break;
            case 'l': o.min_size = atoll(optarg); break;
            case 'h': o.usage = true; break;
            case 'x': break;
            case 'k': o.num_partition_files = atoi(optarg); break;
            case '?': fprintf(stderr, "unrecognised option '%c'\n", (char)optopt); return 1;
            case ':': fprintf(stderr, "argument to option '%c' is missing.\n", (char)optopt); return 1;
        }
    }
    bool ok = true;
    if (o.num_threads <= 0) { fprintf(stderr, "cpu threads must be greater than 0\n"); ok = false; }
    if (o.batch_size <= 0) { fprintf(stderr, "batch size must be greater than 0\n"); ok = false; }
    if (o.min_mapping_ratio < 0.0) { fprintf(stderr, "mapping ratio must be >= 0.0\n"); ok = false; }
    if (o.min_cov < 0) { fprintf(stderr, "coverage must be >= 0\n"); ok = false; }
    if (o.min_cov < 0) { fprintf(stderr, "sequence size must be >= 0\n"); ok = false; }      // (the reference tests min_cov twice, options.cpp:272)
    if (argc < 3) return 1;
    o.input = argv[argc - 3]; o.reads = argv[argc - 2]; o.output = argv[argc - 1];
    return ok ? 0 : 1;
}

double now_s() {
    struct timeval t;
    gettimeofday(&t, NULL);
    return t.tv_sec + 1e-6 * t.tv_usec;
}

struct ScopedTimer {      // DynamicTimer, common/defs.h:175-191
    std::string name;
    double t0;
    explicit ScopedTimer(const std::string& n) : name(n) { fprintf(stderr, "[%s] begins.\n", name.c_str()); t0 = now_s(); }
    ~ScopedTimer() { fprintf(stderr, "[%s] takes %.2f secs.\n", name.c_str(), now_s() - t0); }
};

[[noreturn]] void die(const char* what) {
    fprintf(stderr, "mecat2cns: %s\n", what);
    fflush(stdout);
    exit(1);
}
[[noreturn]] void die_abi(const char* what) {
    fprintf(stderr, "mecat2cns: %s: %s\n", what, mhip_last_error());
    fflush(stdout);
    exit(1);
}

struct PartFile { std::string name; long min_id, max_id; };

std::vector<PartFile> load_index(const std::string& path) {      // load_partition_files_info: name, first and last read id per line
    std::vector<PartFile> v;
    FILE* f = fopen(path.c_str(), "r");
    if (!f) die(("cannot open " + path).c_str());
    char name[4096];
    long a, b;
    while (fscanf(f, "%4095s %ld %ld", name, &a, &b) == 3) v.push_back({name, a, b});
    fclose(f);
    return v;
}

std::vector<mhip_ext_candidate> load_records(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) die(("cannot open " + path).c_str());
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<mhip_ext_candidate> v((size_t)bytes / sizeof(mhip_ext_candidate));
    if (!v.empty() && fread(v.data(), sizeof(mhip_ext_candidate), v.size(), f) != v.size()) die(("read error on " + path).c_str());
    fclose(f);
    return v;
}

// one partition file -> its text appended to `out`
void correct_partition(mhip_ctx* ctx, const mhip_volume* vol, const Options& o, const std::string& path, bool host_text, FILE* out) {
    std::vector<mhip_ext_candidate> recs = load_records(path);
    int64_t dropped[2];
    const std::vector<int64_t> tb = cns_group_templates(recs.data(), recs.size(), o.min_cov, o.min_size, dropped);
    const int nt = (int)tb.size() - 1;
    if (nt == 0) return;
    mhip_cns_opts opts;
    opts.tech = o.tech; opts.input_type = o.input_type; opts.min_align_size = o.min_align_size; opts.min_cov = o.min_cov; opts.min_size = (int)o.min_size;
    opts.num_threads = o.num_threads; opts.want = host_text ? MHIP_CNS_WANT_READS : MHIP_CNS_WANT_TEXT; opts.min_mapping_ratio = o.min_mapping_ratio;
    mhip_cns_outputs res;
    if (mhip_cns_correct_templates(ctx, vol, recs.data(), tb.data(), nt, &opts, &res)) die_abi(path.c_str());
    char* text = res.text;
    int64_t bytes = res.text_bytes;
    if (host_text && mhip_cns_format_reads(res.reads, res.read_begin ? res.read_begin[nt] : 0, res.seq, res.seq_bytes, &text, &bytes)) die_abi(path.c_str());
    if (bytes > 0 && fwrite(text, 1, (size_t)bytes, out) != (size_t)bytes) die("write error on the output file");
    if (host_text) mhip_cns_free(text);
    mhip_cns_outputs_free(&res);
}

}  // namespace

int main(int argc, char** argv) {
    Options o;
    bool filled = false;
    const int refused = parse_arguments(argc, argv, o, &filled);
    if (filled) print_options(o);
    fflush(stdout);
    if (refused) { print_usage(argv[0]); return 1; }
    if (o.usage) { print_usage(argv[0]); return 0; }
    if (o.min_size > 0x3fffffffLL) die("-l is too large");

    if (o.input_type == 0) partition_candidates_text(o.input, (long)o.batch_size, (int)o.min_size, o.num_threads);
    else partition_m4_text(o.input, o.min_mapping_ratio - 0.02, (long)o.batch_size, (int)o.min_size, o.num_threads);      // reads_correction_m4.cpp:79-80
    const std::vector<PartFile> parts = load_index(std::string(o.input) + ".partition_files");

    HostVolume hv;
    {
        ScopedTimer t("load_fasta_db");
        long bad_read = 0;
        const int rc = load_reads_in_memory(o.reads, kMaxSeqSize, &hv, &bad_read);
        if (rc == 1) { fprintf(stderr, "mecat2cns: read %ld has %ld letters or more: not supported (MAX_SEQ_SIZE)\n", bad_read, kMaxSeqSize); return 1; }
        if (rc == 2) { fprintf(stderr, "mecat2cns: the reads do not fit one volume of %ld bases: not supported yet\n", kMaxVolumeBases); return 1; }
    }
    FILE* out = fopen(o.output, "wb");
    if (!out) die((std::string("cannot open ") + o.output + " for writing").c_str());
    if (parts.empty() || hv.num_reads == 0) { fclose(out); return 0; }

    mhip_ctx* ctx = nullptr;
    mhip_volume* vol = nullptr;
    if (mhip_ctx_create(0, nullptr, &ctx)) die_abi("no device");
    if (mhip_volume_upload(ctx, hv.pac.data(), hv.offs.data(), hv.num_reads, hv.num_bases, 0, &vol)) die_abi("volume upload");      // once: resident for all partitions
    const char* ht = getenv("MECAT_CNS_HOST_TEXT");
    const bool host_text = ht && ht[0] == '1';
    for (const PartFile& p : parts) {
        ScopedTimer t("processing " + p.name);
        correct_partition(ctx, vol, o, p.name, host_text, out);
    }
    if (fclose(out) != 0) die("write error on the output file");
    mhip_volume_free(vol);
    mhip_ctx_destroy(ctx);
    return 0;
}
