// table_block_dump.cpp -- lays out, with flake_amd/csrc/table_block.h, the table blocks api.hip builds -- the segment
// tables of fhip_decode_frames_segments in each of its modes and the range tables of fhip_index_frames -- for every
// nsegs (nranges) 0 .. 9 and nstreams 0 .. 3, and prints every slot.  tests/test_table_block_cpu.py checks what is
// printed; built with -fsanitize=address,undefined the program also proves the sizes, for it fills every slot to its
// last byte in a block of exactly the layout's size.  No GPU, no HIP.
//
// Output: per case "C name ns nst total", then per table "S offset bytes element_size".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "table_block.h"

namespace {
struct Row { size_t off, bytes, elem; };

struct Case {
    fhip::TableLayout l;
    std::vector<Row> rows;
    template <class T> void add(size_t count)
    {
        const fhip::TableSlot<T> s = l.add<T>(count);
        rows.push_back(Row{s.off, s.bytes, sizeof(T)});
    }
    void finish(const char *name, size_t ns, size_t nst)
    {
        printf("C %s %zu %zu %zu\n", name, ns, nst, l.bytes());
        unsigned char *block = static_cast<unsigned char *>(malloc(l.bytes()));       // (exactly: one byte more is a report)
        if (!block && l.bytes()) { fprintf(stderr, "out of memory\n"); exit(2); }
        for (size_t k = 0; k < rows.size(); k++) {
            printf("S %zu %zu %zu\n", rows[k].off, rows[k].bytes, rows[k].elem);
            if (rows[k].bytes) memset(block + rows[k].off, (int)(k + 1), rows[k].bytes);
        }
        // no table was written over by a later one
        for (size_t k = 0; k < rows.size(); k++)
            for (size_t i = 0; i < rows[k].bytes; i++)
                if (block[rows[k].off + i] != (unsigned char)(k + 1)) { fprintf(stderr, "table %zu overwritten\n", k); exit(1); }
        free(block);
    }
};

// decode_segments_host's block: the segment tables, K6's CSR with md5, the window tables, the rows tables
void segments(const char *name, size_t ns, size_t nst, bool md5, bool win, bool rows)
{
    Case c;
    c.add<int64_t>(ns); c.add<int64_t>(ns); c.add<int64_t>(ns);
    c.add<int32_t>(ns + 1); c.add<int32_t>(ns); c.add<int32_t>(ns);
    c.add<int32_t>(md5 ? nst + 1 : 0); c.add<int32_t>(md5 ? ns : 0);
    c.add<int64_t>(win ? ns : 0); c.add<int64_t>(win ? ns : 0);
    c.add<int64_t>(rows ? ns : 0); c.add<int32_t>(rows ? ns : 0);
    c.finish(name, ns, nst);
}

// fhip_index_frames' block: range_first, range_consumed, range_frames, range_variable, frame_bytes [fcap]
void index(size_t nr, size_t fcap)
{
    Case c;
    c.add<int64_t>(nr + 1); c.add<int64_t>(nr);
    c.add<int32_t>(nr); c.add<int32_t>(nr); c.add<int32_t>(fcap);
    c.finish("index", nr, fcap);
}
}  // namespace

int main()
{
    for (size_t ns = 0; ns <= 9; ns++) {
        for (size_t nst = 0; nst <= 3; nst++) {
            segments("segments", ns, nst, false, false, false);
            segments("md5", ns, nst, true, false, false);
            segments("windows", ns, nst, false, true, false);
            segments("rows", ns, nst, false, true, true);
        }
        const size_t fcaps[] = {0, 1, 2, 7, 65536, 65539};
        for (size_t fcap : fcaps) index(ns, fcap);
    }
    // the head of a slot: the part of frame_bytes that comes back in the first copy
    fhip::TableLayout l;
    l.add<int64_t>(3);
    const fhip::TableSlot<int32_t> sizes = l.add<int32_t>(11), head = sizes.head(5);
    printf("H %zu %zu %zu %zu\n", sizes.off, sizes.bytes, head.off, head.end());
    return 0;
}
