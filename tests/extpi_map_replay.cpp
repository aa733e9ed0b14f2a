// Host replay of the column -> position map of the extended+i interpolation kernel (hypre_amd/csrc/extpi_map.hpp): the
// same hash, probe and sizes the kernel compiles, on a host array, with the occupant counts the kernel's guard
// (extpi_map_has_room) admits.  Built with -fsanitize=address,undefined by tests/test_extpi_map_replay.py.
//
// For every rung of the ladder:
//   * the largest strong-neighbour count the guard admits leaves exactly one slot free when the interpolatory set is full
//     (strong + capR == capM - 1), and the first count it refuses is the first that could fill the map;
//   * with that many occupants — sequential keys, scattered keys, keys that all hash to one slot; on a zeroed table and
//     on one whose every slot still carries an earlier row's tag — every insertion and every look-up (of present and of
//     absent keys) ends and returns what was stored;
//   * one occupant more (never looked up here: that probe would not end) leaves no free slot.
// A probe that does not end would hang the program: alarm() ends it with a signal instead.
#include "extpi_map.hpp"

#include <cstdio>
#include <cstdlib>
#include <unistd.h>
#include <vector>

using namespace hamd;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

enum { SEQUENTIAL, SCATTERED, ONE_SLOT };

static std::vector<int> distinct_keys(int kind, int count, int mask)
{
   std::vector<int> k;
   k.reserve((size_t) count);
   if (kind == SEQUENTIAL) { for (int i = 0; i < count; i++) { k.push_back(1000 + i); } }
   else if (kind == SCATTERED)
   {
      // a full-period LCG modulo 2^24: no value twice
      unsigned x = 12345u;
      for (int i = 0; i < count; i++) { x = (x * 1664525u + 1013904223u) & 0xffffffu; k.push_back((int) x); }
   }
   else
   {
      for (int c = 0; (int) k.size() < count; c++) { if (((((unsigned) c * 2654435761u) >> 7) & (unsigned) mask) == 5u) { k.push_back(c); } }
   }
   return k;
}

static int slots_of(const std::vector<unsigned long long> &tab, unsigned tag)
{
   int c = 0;
   for (unsigned long long e : tab) { c += (unsigned) (e >> 32) == tag; }
   return c;
}

// strongF strong F neighbours and nset set members go in as the kernel puts them in (a look-up before every set member),
// interleaved; then everything is looked up, with `absent` keys that were never inserted
static void replay(int capR, int capM, int strongF, int nset, int kind, bool stale)
{
   const int mask = capM - 1, absent = 64;
   CHECK(nset <= capR && extpi_map_has_room(strongF, capR, capM), "a replay of counts the kernel never reaches (%d, %d)", strongF, nset);
   std::vector<unsigned long long> tab((size_t) capM, 0ull);
   std::vector<int> val((size_t) capM, 12345);
   unsigned tag = 1;
   if (stale)
   {
      for (int s = 0; s < capM; s++) { tab[(size_t) s] = (7ull << 32) | (unsigned) s; }
      tag = 8;
   }
   const std::vector<int> keys = distinct_keys(kind, strongF + nset + absent, mask);
   std::vector<int> want((size_t) (strongF + nset), 0);
   int f = 0, c = 0, at = 0;
   while (f < strongF || c < nset)
   {
      const bool take_f = f < strongF && (c >= nset || (long long) f * nset <= (long long) c * strongF);
      const int key = keys[(size_t) at];
      if (take_f) { map_set(tab.data(), val.data(), mask, tag, key, STRONG_F); want[(size_t) at] = STRONG_F; f++; }
      else
      {
         CHECK(map_get(tab.data(), val.data(), mask, tag, key) == ABSENT, "key %d present before its insertion", key);
         map_set(tab.data(), val.data(), mask, tag, key, c); want[(size_t) at] = c; c++;
      }
      at++;
   }
   CHECK(slots_of(tab, tag) == strongF + nset, "%d slots for %d occupants", slots_of(tab, tag), strongF + nset);
   for (int q = 0; q < strongF + nset; q++)
   {
      const int got = map_get(tab.data(), val.data(), mask, tag, keys[(size_t) q]);
      CHECK(got == want[(size_t) q], "capM %d kind %d: key %d holds %d, not %d", capM, kind, keys[(size_t) q], got, want[(size_t) q]);
   }
   for (int q = strongF + nset; q < strongF + nset + absent; q++)
   {
      CHECK(map_get(tab.data(), val.data(), mask, tag, keys[(size_t) q]) == ABSENT, "capM %d kind %d: key %d was never inserted", capM, kind, keys[(size_t) q]);
   }
   // a present key set again keeps its slot
   if (strongF + nset > 0)
   {
      map_set(tab.data(), val.data(), mask, tag, keys[0], 77);
      CHECK(map_get(tab.data(), val.data(), mask, tag, keys[0]) == 77, "overwrite lost");
      CHECK(slots_of(tab, tag) == strongF + nset, "an overwrite took a new slot");
   }
}

int main()
{
   alarm(120);
   const int want_slots[EXTPI_RUNGS] = {256, 512, 1024, 4096};
   for (int rung = 0; rung < EXTPI_RUNGS; rung++)
   {
      const int capR = EXTPI_ROOM[rung], capM = extpi_map_slots(capR);
      CHECK(capM == want_slots[rung] && (capM & (capM - 1)) == 0, "rung %d: %d slots", rung, capM);
      int admitted = -1;
      for (int s = 0; s <= 2 * capM; s++)
      {
         const bool ok = extpi_map_has_room(s, capR, capM);
         if (ok) { CHECK(admitted == s - 1, "rung %d: the guard admits %d after refusing a smaller count", rung, s); admitted = s; }
      }
      // the last admitted count leaves one slot free under a full set; the first refused one could fill the map
      CHECK(admitted + capR == capM - 1, "rung %d: last admitted count %d", rung, admitted);
      CHECK(!extpi_map_has_room(admitted + 1, capR, capM) && admitted + 1 + capR == capM, "rung %d: first refused count", rung);
      CHECK(!extpi_map_has_room(0x7fffffff, capR, capM), "rung %d: a huge count", rung);
      for (int kind = SEQUENTIAL; kind <= ONE_SLOT; kind++)
      {
         for (int stale = 0; stale < 2; stale++)
         {
            replay(capR, capM, admitted, capR, kind, stale != 0);        // the fullest map the guard admits: one free slot
            replay(capR, capM, admitted, 0, kind, stale != 0);           // strong F neighbours alone
            replay(capR, capM, admitted / 2, capR / 2, kind, stale != 0);
            replay(capR, capM, 0, capR, kind, stale != 0);
            replay(capR, capM, 1, 0, kind, stale != 0);
         }
      }
      // one more occupant: no slot left, so the next probe for an absent key would have nowhere to stop
      {
         const int mask = capM - 1;
         std::vector<unsigned long long> tab((size_t) capM, 0ull);
         std::vector<int> val((size_t) capM, 0);
         const std::vector<int> keys = distinct_keys(SCATTERED, capM, mask);
         for (int q = 0; q < admitted + 1 + capR; q++) { map_set(tab.data(), val.data(), mask, 1u, keys[(size_t) q], q); }
         CHECK(slots_of(tab, 1u) == capM, "rung %d: %d occupants leave %d slots free", rung, admitted + 1 + capR, capM - slots_of(tab, 1u));
      }
      printf("rung %d: tables for %d entries, map of %d slots, strong neighbours admitted up to %d\n", rung, capR, capM, admitted);
   }
   if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
   printf("extpi map replay ok\n");
   return 0;
}
