/* ref_harness_asmpw_ext.c — TEST INFRASTRUCTURE: the extension loop of the UNMODIFIED mecat2asmpw.c, column by column.
 *
 * pairwise_mapping (mecat2asmpw.c:514-959) keeps the aligned strings of a candidate in locals: left_store1 / left_store2 / right_store1 /
 * right_store2, consecutive equal-sized members of one heap struct (output_store, :64-67).  Once per candidate, in list order, after both
 * directions have finished and before anything edits the strings, it calls the external function
 *     string_check(out_store1, out_store2, left_store1, left_store2)                                                       (:859)
 * so the two pointers it passes locate all four stores: with w = str2 - str1 the right pair lies at str1 + 2 w and str1 + 3 w.  As in
 * ref_harness_asmpw_cand.c the reference file is compiled as it lies into its own object (oracle/Makefile: main renamed on the command
 * line, nothing else), the symbol `string_check` of that object is made weak (objcopy) and this file supplies the one the object then
 * calls: it copies the four strings and returns.  (Not forwarding the call leaves the left pair unshuffled, which changes only the lines
 * the tool prints — to /dev/null here.)  Everything else — seeding, candidate selection, `align`, the block loop, the tail cut, the
 * failure and drop rules — runs as the reference wrote it.
 * store1 = the subject's row (the indexed block: `align`'s query_seq, :757 / :809), store2 = the mapped read's row; both in extension
 * order (the left pair outwards from the last base of the seed 13-mer, :741-747).
 * tests/golden/make_golden_asm_ext.py turns the strings into tests/golden/asm_ext.npz.  Never linked by the product path. */
#include <malloc.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* the reference's file-scope state (mecat2asmpw.c:71-81), external linkage there */
typedef struct { int readno, readlen; char* seqloc; } ReadFasta;
typedef struct { int readno, length; char* mem; } readmemory;
extern pthread_mutex_t mutilock;
extern int runnumber, runthreadnum, readcount, terminalnum;
extern int *countin, **databaseindex, *allloc, sumcount;
extern int seed_len, *llocation, seqcount, curreadcount;
extern char* STRMEM;
extern readmemory* indexread;
extern ReadFasta* readinfo;
extern FILE** outfile;
void creat_ref_index(char* seq, int seqcount);
void pairwise_mapping(int threadint);

static char* g_rec = NULL;
static long g_cap = 0, g_used = 0;
static int g_calls = 0, g_overflow = 0;

/* the `string_check` the reference object calls: one record per candidate = four int32 lengths (left_store1, left_store2, right_store1,
 * right_store2), then the four strings without their NULs */
void string_check(char* seq1, char* seq2, char* str1, char* str2) {
    const long w = str2 - str1;
    const char* s[4];
    int len[4], i;
    long need = 16;
    (void)seq1; (void)seq2;
    s[0] = str1; s[1] = str2; s[2] = str1 + 2 * w; s[3] = str1 + 3 * w;
    for (i = 0; i < 4; ++i) { len[i] = (int)strlen(s[i]); need += len[i]; }
    if (g_used + need > g_cap) { g_overflow = 1; return; }
    memcpy(g_rec + g_used, len, 16);
    g_used += 16;
    for (i = 0; i < 4; ++i) { memcpy(g_rec + g_used, s[i], (size_t)len[i]); g_used += len[i]; }
    ++g_calls;
}

static ReadFasta g_query;
static FILE* g_null = NULL;

/* The block the tool indexes, as load_read leaves it (:388-409): text = the reads in upper case, one NUL after each; starts[i] = offset
 * of read i; n = bytes.  llocation has one more entry than reads, which load_read never writes: the tool reads it for the last read
 * of the block (:640) and finds what malloc returned, zero on a fresh heap — zero here.  (Same set-up as refasmc_setup.)
 * pairwise_mapping reads parts of its malloc'ed segment array that it never wrote (the sweeps of :693-707 index loczhi[] / seedno[] by a
 * count that can pass what was stored), so which candidates it keeps, and in which order, can depend on what earlier calls left on the
 * heap.  glibc's M_PERTURB with 0xFF hands every allocation out filled with 0x00 — the state of a fresh heap, which is also what the
 * restatement's fresh mode (asm_block_fresh) and the device path define — so a call does not depend on the calls before it.  The
 * setting is process-wide: both entry points switch it on for their own duration only and leave the allocator as they found it
 * (M_PERTURB is 0 unless a caller set it), so nothing else in the process runs on a perturbed heap. */
int refasme_setup(char* text, int n, const int* starts, const int* lens, int nreads, int first_readno) {
    int i;
    mallopt(M_PERTURB, 0xFF);
    seed_len = 13;
    STRMEM = text;
    seqcount = n;
    curreadcount = nreads;
    free(llocation);
    free(indexread);
    llocation = (int*)calloc((size_t)nreads + 1, sizeof(int));
    indexread = (readmemory*)calloc((size_t)nreads + 1, sizeof(readmemory));
    for (i = 0; i < nreads; ++i) {
        llocation[i] = starts[i];
        indexread[i].mem = text + starts[i];
        indexread[i].readno = first_readno + i;
        indexread[i].length = lens[i];
    }
    free(countin); free(allloc); free(databaseindex);
    creat_ref_index(STRMEM, seqcount);
    if (!g_null) g_null = fopen("/dev/null", "w");
    if (!outfile) outfile = (FILE**)malloc(sizeof(FILE*));
    outfile[0] = g_null;
    if (!readinfo) readinfo = &g_query;
    pthread_mutex_init(&mutilock, NULL);
    mallopt(M_PERTURB, 0);
    return sumcount;
}

/* the store strings of every candidate of one query read (upper-case text, NUL-terminated), in list order.  Returns the number of
 * candidates (string_check calls), or -1 when `cap` bytes were not enough. */
int refasme_extend(char* query, int read_name, char* rec, long cap, long* used) {
    g_rec = rec; g_cap = cap; g_used = 0; g_calls = 0; g_overflow = 0;
    readinfo = &g_query;
    g_query.readno = read_name;
    g_query.readlen = (int)strlen(query);
    g_query.seqloc = query;
    readcount = 1;
    terminalnum = 1;
    runnumber = 0;
    runthreadnum = 0;
    mallopt(M_PERTURB, 0xFF);
    pairwise_mapping(0);
    mallopt(M_PERTURB, 0);
    *used = g_used;
    return g_overflow ? -1 : g_calls;
}
