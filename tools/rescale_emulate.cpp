// tools/rescale_emulate.cpp -- the quality rescale (pss-bam_amd/csrc/rescale_kernels.h) compiled for the host: the per-record
// function, inside the loop a kernel of the record sink's path would run around it -- offs[] of the input block, a scanned dst[] with
// an entry per input record, dropped records (dst[r] == dst[r + 1]) between the kept ones, one "lane" after the other.
//
//     g++ -O1 -I pss-bam_amd/csrc -o rescale_emulate tools/rescale_emulate.cpp
//     ./rescale_emulate in.raw genome.bin table.bin out.raw ds <D> <region_len> <min_mapq>
//
// in.raw holds BAM records back to back (le32 block_size + body: a submitted block); genome.bin the BAM's references in refID
// order, each as le32 length + that many letters (length 0xFFFFFFFF: the genome lacks it); table.bin the 2 * rows * 94 bytes of the
// table (host/rescale.h builds one).  A record is kept when pssbam_rescale_host_plan -- pss-bam -r <region_len> -q <min_mapq>,
// everything else at its default -- adds it to a table; out.raw receives the kept records, rescaled, and stdout the counters, a line
// per end and row.  tests/test_rescale_host.py runs it.  The input block, the output and every contig live in heap blocks of exactly
// their size, so that built with -fsanitize=address,undefined a write outside the output, or a read outside any of them, is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rescale_kernels.h"

static bool slurp(const char *path, std::vector<uint8_t> &v) {
    FILE *in = fopen(path, "rb");
    if (!in) { fprintf(stderr, "rescale_emulate: cannot open %s\n", path); return false; }
    uint8_t buf[1 << 16];
    for (size_t n; (n = fread(buf, 1, sizeof buf, in)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(in);
    return true;
}

int main(int argc, char **argv) {
    if (argc != 9) { fprintf(stderr, "usage: rescale_emulate in.raw genome.bin table.bin out.raw ds|ss D region_len min_mapq\n"); return 2; }
    const uint32_t mode = !strcmp(argv[5], "ds") ? PSSBAM_RS_DS : !strcmp(argv[5], "ss") ? PSSBAM_RS_SS : PSSBAM_RS_OFF;
    const unsigned long D = strtoul(argv[6], nullptr, 10), region_len = strtoul(argv[7], nullptr, 10), min_mq = strtoul(argv[8], nullptr, 10);
    std::vector<uint8_t> raw_v, gen, tab_v;
    if (!slurp(argv[1], raw_v) || !slurp(argv[2], gen) || !slurp(argv[3], tab_v)) return 1;
    const size_t rows = tab_v.size() / (2u * PSSBAM_RS_QUALS);
    if (mode == PSSBAM_RS_OFF || rows < 1 || rows > PSSBAM_RS_MAX_ROWS || tab_v.size() != rows * 2u * PSSBAM_RS_QUALS || D < 1 || D > rows || D > region_len) {
        fprintf(stderr, "rescale_emulate: bad mode, table size or D\n");
        return 2;
    }
    // the contigs in the genome's stored form, each in a block of its own
    std::vector<uint8_t *> contigs;
    std::vector<uint32_t> contig_len;
    for (size_t at = 0; at < gen.size();) {
        if (gen.size() - at < 4) { fprintf(stderr, "rescale_emulate: genome.bin ends inside a length\n"); return 1; }
        const uint32_t len = pssbam_rs_u32(gen.data() + at);
        at += 4;
        if (len == 0xFFFFFFFFu) { contigs.push_back(nullptr); contig_len.push_back(0); continue; }
        if (len > gen.size() - at) { fprintf(stderr, "rescale_emulate: genome.bin ends inside a contig\n"); return 1; }
        uint8_t *c = (uint8_t *)malloc(len ? len : 1);
        if (!c) return 1;
        for (uint32_t j = 0; j < len; j++) {
            const int b = gen[at + j] >= 'a' && gen[at + j] <= 'z' ? gen[at + j] - 32 : gen[at + j];
            c[j] = (uint8_t)(b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : b);
        }
        contigs.push_back(c);
        contig_len.push_back(len);
        at += len;
    }
    uint8_t *raw = (uint8_t *)malloc(raw_v.size() ? raw_v.size() : 1), *table = (uint8_t *)malloc(tab_v.size());
    if (!raw || !table) return 1;
    memcpy(raw, raw_v.data(), raw_v.size());
    memcpy(table, tab_v.data(), tab_v.size());
    // offs[] of the block, and len[] as select_mark leaves it, scanned into dst[]
    struct Kept { const uint8_t *G; int64_t s; uint32_t L, rev, in_fwd, in_rev; };
    std::vector<uint32_t> offs, dst;
    std::vector<Kept> plan;
    size_t at = 0, total = 0;
    for (uint32_t r = 0; at < raw_v.size(); r++) {
        if (raw_v.size() - at < 4) { fprintf(stderr, "rescale_emulate: %zu stray bytes at the end\n", raw_v.size() - at); return 1; }
        const uint64_t len = 4ull + pssbam_rs_u32(raw + at);
        if (len > raw_v.size() - at) { fprintf(stderr, "rescale_emulate: record %u leaves the stream\n", r); return 1; }
        Kept k{};
        const int keep = pssbam_rescale_host_plan(raw + at, (uint32_t)len, contigs.data(), contig_len.data(), (int32_t)contigs.size(), (uint32_t)region_len,
                                                  (uint32_t)min_mq, &k.G, &k.s, &k.L, &k.rev, &k.in_fwd, &k.in_rev);
        offs.push_back((uint32_t)at);
        dst.push_back((uint32_t)total);
        plan.push_back(k);
        if (keep) total += (size_t)len;
        at += (size_t)len;
    }
    offs.push_back((uint32_t)at);
    dst.push_back((uint32_t)total);
    const uint32_t n = (uint32_t)offs.size() - 1u;
    uint8_t *out = (uint8_t *)malloc(total ? total : 1);   // exactly the kept records: no slack for a stray byte
    if (!out) return 1;
    for (uint32_t r = 0; r < n; r++)                       // select_gather
        if (dst[r + 1u] > dst[r]) memcpy(out + dst[r], raw + offs[r], dst[r + 1u] - dst[r]);
    std::vector<uint32_t> counts(4u * rows, 0u);
    for (uint32_t r = 0; r < n; r++) {                     // the rescale, a lane after the other
        const uint32_t d0 = dst[r], d1 = dst[r + 1u];
        if (d1 <= d0 || d1 > total) continue;
        const uint32_t o0 = offs[r], o1 = offs[r + 1u];
        if (o1 - o0 != d1 - d0) continue;
        const Kept &k = plan[r];
        pssbam_rescale_record(raw + o0, out + d0, d1 - d0, k.G, k.s, k.L, k.rev, k.in_fwd, k.in_rev, mode, (uint32_t)D, (uint32_t)rows, 0u, table, counts.data());
    }
    for (uint32_t end = 0; end < 2u; end++)
        for (uint32_t i = 0; i < D; i++)
            printf("%u\t%u\t%u\t%u\n", end ? 3u : 5u, i, counts[(end * rows + i) * 2u], counts[(end * rows + i) * 2u + 1u]);
    FILE *o = fopen(argv[4], "wb");
    if (!o || fwrite(out, 1, total, o) != total) { fprintf(stderr, "rescale_emulate: cannot write %s\n", argv[4]); return 1; }
    free(out);
    free(raw);
    free(table);
    for (uint8_t *c : contigs) free(c);
    return fclose(o) ? 1 : 0;
}
