// hypre_amd — the column -> position map of the extended+i interpolation kernel (interp_kernels.hip): hash, probe and the
// sizes of the retry ladder, in plain C++ so that a host program can replay them (tests/extpi_map_replay.cpp).
//
// The map is an open-addressing table of capM slots (a power of two).  A slot is (tag << 32 | key); a row owns the slots
// that carry its tag, everything else — zeroed slots, slots of earlier rows — is free.  A probe stops at a free slot or
// at its own key and at nothing else: it terminates only while the row leaves at least one slot free.  The occupants of a
// row are its strong F neighbours (one entry each, no count check on insertion) and its interpolatory set (at most capR
// entries, checked on insertion), so a row with `strong` strong neighbours holds at most strong + capR of them and
// extpi_map_has_room() is the whole termination argument: a row that fails it is not started.
#ifndef HYPRE_AMD_EXTPI_MAP_HPP
#define HYPRE_AMD_EXTPI_MAP_HPP

#if defined(__HIPCC__)
#define HAMD_MAP_FN __device__ __forceinline__
#define HAMD_MAP_BOTH __host__ __device__ __forceinline__
#else
#define HAMD_MAP_FN inline
#define HAMD_MAP_BOTH inline
#endif

namespace hamd {

constexpr int ABSENT = -1, STRONG_F = -2;

// interpolatory-set entries per row on the four rungs of the ladder, and the slots of the map that goes with them
constexpr int EXTPI_RUNGS = 4;
constexpr int EXTPI_ROOM[EXTPI_RUNGS] = {64, 128, 256, 1024};
HAMD_MAP_BOTH int extpi_map_slots(int capR) { int p = 16; while (p < 4 * capR) { p <<= 1; } return p; }

// May a row with `strong` entries in S be started with tables for capR set members and a map of capM slots?  Its
// occupants number at most strong + capR; one slot must stay free.
HAMD_MAP_BOTH bool extpi_map_has_room(int strong, int capR, int capM) { return strong < capM - capR; }

// the one atomic of the map: lanes of a wave insert distinct keys side by side and may meet in a slot
#if defined(__HIPCC__)
HAMD_MAP_FN unsigned long long map_cas(unsigned long long *slot, unsigned long long expect, unsigned long long v) { return atomicCAS(slot, expect, v); }
#else
HAMD_MAP_FN unsigned long long map_cas(unsigned long long *slot, unsigned long long expect, unsigned long long v)
{ const unsigned long long old = *slot; if (old == expect) { *slot = v; } return old; }
#endif

HAMD_MAP_FN int map_get(const unsigned long long *tab, const int *val, int mask, unsigned tag, int key)
{
   unsigned h = ((unsigned) key * 2654435761u) >> 7;
   while (true)
   {
      const unsigned long long e = tab[h & mask];
      if ((unsigned) (e >> 32) != tag) { return ABSENT; }
      if ((int) (unsigned) e == key) { return val[h & mask]; }
      h++;
   }
}

// insert a key known to be absent, or overwrite the value of a present one (lanes work on distinct keys)
HAMD_MAP_FN void map_set(unsigned long long *tab, int *val, int mask, unsigned tag, int key, int v)
{
   unsigned h = ((unsigned) key * 2654435761u) >> 7;
   const unsigned long long mine = ((unsigned long long) tag << 32) | (unsigned) key;
   while (true)
   {
      const unsigned long long e = tab[h & mask];
      if ((unsigned) (e >> 32) != tag)
      {
         if (map_cas(&tab[h & mask], e, mine) == e) { val[h & mask] = v; return; }
         continue;
      }
      if ((int) (unsigned) e == key) { val[h & mask] = v; return; }
      h++;
   }
}

}  // namespace hamd

#endif
