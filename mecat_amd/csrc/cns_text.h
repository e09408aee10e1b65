// cns_text.h — the corrected reads' FASTA text (cns_text.hip): what the host and the device share.
//
// A record's text is reads_correction_can.cpp:44-46: ">" read_id "_" range_beg "_" range_end "_" size, newline, the `size` letters,
// newline.  The header's character rule is one function, cns_text_header_char: the text kernel calls it with the lane number (lane l
// writes character l of the header: at most 45 characters, no serial itoa), and libcns_poa_host.so exports it compiled by plain g++
// (cns_text_host_*), so that tests/test_cns_text_ref_cpu.py reaches the code the kernel runs.  The four numbers are not negative.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CNS_TEXT_HD __host__ __device__
#else
#define CNS_TEXT_HD
#endif

enum { CNS_TEXT_MAX_HEADER = 45 };      // '>' + four numbers of at most 10 digits + three '_' + newline

// decimal digits of v >= 0
CNS_TEXT_HD inline int cns_text_digits(int32_t v) {
    int d = 1;
    for (uint32_t x = (uint32_t)v; x >= 10u; x /= 10u) ++d;
    return d;
}

// characters of the header line, its newline included
CNS_TEXT_HD inline int cns_text_header_len(int32_t read_id, int32_t range_beg, int32_t range_end, int32_t size) {
    return 5 + cns_text_digits(read_id) + cns_text_digits(range_beg) + cns_text_digits(range_end) + cns_text_digits(size);
}

// characters of the whole record: header line, letters, newline
CNS_TEXT_HD inline long long cns_text_record_len(int32_t read_id, int32_t range_beg, int32_t range_end, int32_t size) {
    return (long long)cns_text_header_len(read_id, range_beg, range_end, size) + size + 1;
}

// character l (0 <= l) of the header line; 0 behind its newline
CNS_TEXT_HD inline char cns_text_header_char(int32_t read_id, int32_t range_beg, int32_t range_end, int32_t size, int l) {
    if (l < 0) return 0;
    if (l == 0) return '>';
    --l;
    const int32_t v[4] = {read_id, range_beg, range_end, size};
    for (int f = 0; f < 4; ++f) {
        const int d = cns_text_digits(v[f]);
        if (l < d) {
            uint32_t x = (uint32_t)v[f];
            for (int k = d - 1 - l; k > 0; --k) x /= 10u;
            return (char)('0' + x % 10u);
        }
        l -= d;
        if (l == 0) return f < 3 ? '_' : '\n';
        --l;
    }
    return 0;
}

#if defined(__HIPCC__)
#include "common.h"

// One launch's text on the device: nreads records' text one behind the other, in record order.
struct CnsTextDev {
    const char* d_text = nullptr;           // [bytes]
    const long long* d_bad = nullptr;       // nonzero once the kernels have run: a record leaves `seq` or holds a negative number, or the
                                            // bytes written are not the bytes counted (NULL: nothing ran)
    long long bytes = 0;
    double wait_s = 0;                      // host seconds spent in the wait for the total
};

// The text of d_reads[nreads], whose seq_begin count into d_seq[seq_bytes] (a buffer that begins on a 16-byte boundary and has 16 bytes
// of room behind seq_bytes: the copy reads whole aligned 16-byte words).  Everything runs on c->stream behind what the stream holds; the
// function WAITS for the stream once (the total sizes the output) and returns with the last kernel launched.  `set` picks the buffers.
int cns_text_launch(mhip_ctx* c, int set, const mhip_cns_read* d_reads, long long nreads, const char* d_seq, long long seq_bytes, CnsTextDev* out);
#endif
