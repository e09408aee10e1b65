// ref_genome.cpp — see ref_genome.h
#include "ref_genome.h"

#include <ctype.h>
#include <stdio.h>

namespace {

const int64_t kMaxBases = 0x7fffffff - 4096;      // int32 positions, with room for the segment arithmetic behind the last base

inline int code_of(unsigned char c) {
    switch (c) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': return 3;
        default: return 4;
    }
}

void put_long(std::string& s, int64_t v) {
    char b[32];
    snprintf(b, sizeof(b), "%lld", (long long)v);
    s += b;
}

}  // namespace

bool ref_genome_parse(const char* text, size_t n, RefGenome* g, std::string* err) {
    *g = RefGenome();
    std::vector<unsigned char> letters;
    letters.reserve(n);
    int64_t rsize = 0;
    size_t i = 0;
    while (i < n) {
        unsigned char ch = (unsigned char)text[i++];
        if (ch == '>') {
            // the rest of the line is the header; the tool demands a non-empty one
            size_t e = i;
            while (e < n && text[e] != '\n') ++e;
            if (e == i) { *err = "reference: a record without a name"; return false; }
            size_t ne = i;
            while (ne < e && text[ne] != ' ' && text[ne] != '\t') ++ne;
            // (the size of the record before goes in front of the new line's fields; an empty record writes none, as in the tool)
            if (rsize) { put_long(g->chrindex, rsize); g->chrindex += '\n'; }
            if (!g->chroms.empty()) g->chroms.back().size = rsize;
            rsize = 0;
            RefChrom c;
            c.start = (int64_t)letters.size();
            c.name.assign(text + i, ne - i);
            put_long(g->chrindex, c.start);
            g->chrindex += '\t';
            g->chrindex += c.name;
            g->chrindex += '\t';
            g->chroms.push_back(c);
            i = e;
        } else if (ch != '\n' && ch != '\r') {
            if (ch > 'Z' && ch < 0x80) ch = (unsigned char)toupper(ch);
            letters.push_back(ch);
            ++rsize;
        }
    }
    if (g->chroms.empty()) { *err = "reference: no FASTA record"; return false; }
    g->chroms.back().size = rsize;
    put_long(g->chrindex, rsize);
    g->chrindex += '\n';
    put_long(g->chrindex, (int64_t)letters.size());
    g->chrindex += "\tFileEnd\n";
    const int64_t nb = (int64_t)letters.size();
    if (nb == 0) { *err = "reference: no sequence letters"; return false; }
    if (nb > kMaxBases) {
        char b[160];
        snprintf(b, sizeof(b), "reference: %lld letters do not fit one volume (int32 positions, at most %lld)", (long long)nb, (long long)kMaxBases);
        *err = b;
        return false;
    }
    g->num_bases = nb;
    g->pac.assign((size_t)(nb + 3) / 4, 0);
    g->nplane.assign((size_t)(nb + 3) / 4, 0);
    int64_t p = 0;
    while (p < nb) {
        int64_t j = p;
        for (; j < nb; ++j) {
            const int c = code_of(letters[(size_t)j]);
            if (c == 4) break;
            g->pac[(size_t)j >> 2] |= (uint8_t)(c << ((~j & 3) << 1));
        }
        if (j > p || p == 0) g->reads.push_back(mhip_offset_t{(int32_t)p, (int32_t)(j - p)});
        if (j == nb) break;
        int64_t e = j;
        for (; e < nb && code_of(letters[(size_t)e]) == 4; ++e) g->nplane[(size_t)e >> 2] |= (uint8_t)(3 << ((~e & 3) << 1));
        // the stretch [j, e) of other letters: j is the end of the read in front of it
        int64_t q = j;
        while (q + 13 < e - 1) {
            q += 13;
            g->reads.push_back(mhip_offset_t{(int32_t)q, 0});
        }
        if (e - 1 > q) g->reads.push_back(mhip_offset_t{(int32_t)(e - 1), 0});
        p = e;
    }
    return true;
}

bool ref_genome_load(const char* path, RefGenome* g, std::string* err) {
    FILE* f = fopen(path, "rb");
    if (!f) { *err = std::string("reference: cannot open ") + path; return false; }
    std::string text;
    char buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, k);
    fclose(f);
    return ref_genome_parse(text.data(), text.size(), g, err);
}

int ref_genome_upload(mhip_ctx* ctx, const RefGenome& g, mhip_volume** vol, mhip_index** idx) {
    *vol = nullptr;
    *idx = nullptr;
    if (mhip_volume_upload(ctx, g.pac.data(), g.reads.data(), (int)g.reads.size(), (int)g.num_bases, 0, vol)) return -1;
    if (mhip_volume_set_nplane(ctx, *vol, g.nplane.data()) || mhip_index_build(ctx, *vol, idx)) {
        mhip_volume_free(*vol);
        *vol = nullptr;
        return -1;
    }
    return 0;
}
