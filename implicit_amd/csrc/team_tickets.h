// Ticket bookkeeping of the chained CG launches (als_cg_qfteam_chain_kernel and als_cg_qfwide_chain_kernel, als_cg_qf.hip): pure
// host arithmetic (no device code, no HIP header), so that it can be read and tested without a GPU (imp_host_chain_tickets,
// imp_host_wide_tickets).
//
// Inside a class of the chain the teams draw their rows by ticket.  One counter for a whole class does not work: every row
// of the device would add to one address, and atomics on one address are served one after the other (measured: 150 K draws
// per half sweep on one counter per class took the configs[2] step from 4.0 to 5.4 ms).  A class is therefore dealt to
// kQueues = 8 queues -- row k of the class (longest first) belongs to queue k mod 8, workgroup b serves queue b mod 8, which
// is its XCD -- with a counter each, a cache line apart.  The queues are equally long and equally heavy to within one row.
//
// On a queue of `count` rows served by N teams, tickets 0 .. 4 N - 1 are dealt out statically -- team g starts with g, g + N,
// g + 2 N, g + 3 N, the four rows its metadata pipeline holds -- and every ticket from 4 N on is one atomic increment of the
// queue's device counter.  The counters are never reset: a launch is told the value each counter has at its start (its
// base) and uses `counter - base`; the host advances the base by the number of draws the launch makes, which the protocol
// fixes:
//   * a team draws once per row it solves, as long as the newest ticket it holds is inside the queue;
//   * so the tickets of [4 N, count) are all drawn, each once, and every team whose static tickets all lie inside the queue
//     (g + 3 N < count) draws exactly one ticket at or past the end, after which it stops drawing.
// All arithmetic on counters and bases is modulo 2^32; a class holds fewer than 2^30 rows (kMaxCount), so `counter - base`
// is exact however often the counter has wrapped.
#ifndef IMPLICIT_AMD_CSRC_TEAM_TICKETS_H_
#define IMPLICIT_AMD_CSRC_TEAM_TICKETS_H_

#include <algorithm>
#include <cstdint>

namespace imp {

// NC classes in one launch: ChainTickets (below) for the three 512-thread classes, WideTickets for the two 1024-thread ones
template <int NC> struct TicketClasses {
  static constexpr int kClasses = NC;
  static constexpr int kQueues = 8;                // queues per class
  static constexpr int kCounterStride = 64;        // words between two device counters: a cache line of their own each
  static constexpr int32_t kMaxCount = 1 << 30;    // a ticket travels in the upper 30 bits of a team's control word
  uint32_t next[kClasses][kQueues] = {};           // what the device counters read once everything queued so far has run

  // rows of queue q of a class of `count` rows: k = q, q + 8, ...
  static int32_t queue_rows(int32_t count, int q) { return count > q ? (count - q + kQueues - 1) / kQueues : 0; }
  // workgroups of a grid that serve queue q: b = q, q + 8, ...
  static int32_t queue_workgroups(int32_t workgroups, int q) { return queue_rows(workgroups, q); }
  // atomic draws of one launch on a queue of `count` rows with `teams` teams
  static uint32_t draws(int32_t count, int32_t teams) {
    if (count <= 0 || teams <= 0) return 0u;  // nobody enters an empty queue
    const int64_t n = teams, c = count;
    const int64_t inside = std::max<int64_t>(0, c - 4 * n);                       // tickets of [4 N, count)
    const int64_t past = std::min<int64_t>(n, std::max<int64_t>(0, c - 3 * n));   // teams with g + 3 N < count
    return (uint32_t)(inside + past);
  }
  // the bases of the next launch -- `workgroups` in the grid, teams_per_workgroup[c] teams of class c in each -- and `next`
  // advanced past its draws
  void launch(const int32_t (&count)[kClasses], int32_t workgroups, const int32_t (&teams_per_workgroup)[kClasses],
              uint32_t (&base)[kClasses][kQueues]) {
    for (int c = 0; c < kClasses; ++c)
      for (int q = 0; q < kQueues; ++q) {
        base[c][q] = next[c][q];
        next[c][q] += draws(queue_rows(count[c], q), queue_workgroups(workgroups, q) * teams_per_workgroup[c]);  // modulo 2^32
      }
  }
};

typedef TicketClasses<3> ChainTickets;  // team widths 8, 4, 2 (als_cg_qfteam_chain_kernel)

// The chained 1024-thread classes (als_cg_qfwide_chain_kernel): class 0 is (256,512], a team of 16 wavefronts -- the workgroup
// -- per row; class 1 are the short rows, whose ticketed unit is a GROUP of kGroupRows consecutive schedule rows that a
// workgroup solves in lock step.  Both have one team per workgroup, and the protocol above holds with "row" read as "group".
struct WideTickets : TicketClasses<2> {
  static constexpr int kGroupRows = 16;
  static int32_t groups(int32_t rows) { return rows > 0 ? (rows + kGroupRows - 1) / kGroupRows : 0; }
  // rows[0]: rows of (256,512], rows[1]: short rows
  void launch_rows(const int32_t (&rows)[2], int32_t workgroups, uint32_t (&base)[2][kQueues]) {
    const int32_t units[2] = {rows[0], groups(rows[1])}, teams[2] = {1, 1};
    launch(units, workgroups, teams, base);
  }
};

}  // namespace imp

#endif  // IMPLICIT_AMD_CSRC_TEAM_TICKETS_H_
