// table_block.h -- the layout of several typed tables in one block of memory.  api.hip uploads a call's small tables
// in one copy and keeps its device-only scratch tables in one allocation; where each table begins in such a block is
// worked out here, once, so that the host image and the device pointer of a table cannot disagree.  No HIP: the layout
// is tested on the CPU (tests/test_table_block_cpu.py).
//
// Tables are added in order and each gets a SLOT: its byte offset in the block and its size in bytes, with the element
// type in the slot's own type.  Every slot begins on an 8-byte boundary, which suits every element of up to 8 bytes; a
// table of no elements is a slot of no bytes.  When the last table is in, bytes() is the size of the block.
#ifndef FHIP_TABLE_BLOCK_H
#define FHIP_TABLE_BLOCK_H

#include <cstddef>

namespace fhip {

template <class T> struct TableSlot {
    size_t off = 0, bytes = 0;
    size_t end() const { return off + bytes; }
    TableSlot head(size_t count) const { return TableSlot{off, count * sizeof(T)}; }     // its first count elements
};

class TableLayout {
    size_t total_ = 0;

public:
    static constexpr size_t ALIGN = 8;
    template <class T> TableSlot<T> add(size_t count)
    {
        static_assert(sizeof(T) <= ALIGN && ALIGN % sizeof(T) == 0, "a slot's boundary must suit its element");
        const TableSlot<T> s{total_, count * sizeof(T)};
        total_ += (s.bytes + ALIGN - 1) / ALIGN * ALIGN;
        return s;
    }
    size_t bytes() const { return total_; }
    size_t words() const { return total_ / ALIGN; }     // the block as 8-byte words
};

}  // namespace fhip

#endif
