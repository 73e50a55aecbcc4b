"""GPU: every call that runs on a caller's device workspace, on a workspace ANY other call left behind.

include/modgpu.h promises that the workspace is "reset by the call's first kernel in stream order" and that modgpu_table_status reports
"whichever kind of table call ran last on the workspace": one scratch buffer per stream may be handed to all of these calls in turn.
Here one buffer W is: the ten kinds of tests/workspace_reuse.py (the five table calls, the two fused ones on every side, the two moving
ones, the single move) and, as a reader, modgpu_digest_check_device.  Every call gets exactly what its own *_workspace_bytes function
returns, at an address inside W, and after every call W outside that range must hold what it held before.  Every case compares all the
call may change with models from outside the library (oracle.cycle_at, zlib.adler32, a numpy compare, the move tests' model): the whole
arena window with its 0xA5 guards, the records between guards of their own, table_status, verify_table_summary, rekey_move_table_status
or move_status, and the launch count.  The calls run in the testing flavour with every stream and move grid forced to 4.

  a  fills       every kind at n in {1, 16, 17, 256, 257, 1025, 4097} on W filled with 0x00, with what ANOTHER kind left after 4097
                 entries, with 0xFF, with seeded random bytes -- a1 to a4, in that order; the last two run for a kind only if it passed
                 the first two
  b  pairs       every ordered pair of kinds: previous at 4097 then next at 17, previous at 17 then next at 4097, W untouched in between
  c  refusals    a refused previous (flags != 0 in entry 123) then a clean next of another kind, and a clean previous then a refused next
  d  readers     verify_table_summary of a small call behind a large one; rekey_move_table_status on each fill; the digest check's
                 read of the producer's header
  e  alignment   every kind with its workspace at an address that is 8 modulo 64, on the leftover fill
  f  graph       cycle_digest_table, rekey_move_table, verify_table captured in one chain on one W, replayed with entries rewritten

No kernel with a reset taken out is built or run (a missing pad can send a descent past the table).  Instead, every workspace word
that a later launch reads, the launch that resets or first writes it, the fill under which a missing reset would change an output,
and the case that applies that fill -- from cycle_table_kernel.h / .hip, cycle_rekey_move_table_kernel.h / .hip, cycle_verify_table_kernel.h /
.hip, cycle_table_impl.h and the host layout in modgpu_capi.cpp:

  field                      reset / first written by                 a missing reset shows under                              case
  CycleTableHdr.ticket       plan, thread 0 of workgroup 0            any nonzero value: the stream kernel's tickets start       a2 a3 a4, b
                             (stream launch adds to it)               past chunk 0, chunks are never cycled.  0x00 hides it;
                                                                      every previous call leaves total + grid there
  CycleTableHdr.pad0         never read by a three-launch kind        (is MoveTableHdr.stalled, below)                          --
  CycleTableHdr.first_bad    plan (~0), lowered by finish             any value but ~0: the status names an entry of a clean     a1 a2 a4, c
                                                                      call (0x00: entry 0; a refused previous: its entry);
                                                                      0xFF hides it
  CycleTableHdr.total        plan (0), finish always stores it        read only behind finish's store: none (pinned anyway: a    a, c
                                                                      refused call must leave 0 for its stream launch)
  CycleTableHdr.pad1         never read by a three-launch kind        (pad1[0] is MoveTableHdr.up, below)                       --
  MoveTableHdr.ticket        plan of each sweep                       as CycleTableHdr.ticket, for the move launch's positions   a2 a3 a4, b
  MoveTableHdr.stalled       plan, except sweep 1 of a relayout       any nonzero value: the status reports a stall, sweep 1     a3 a4, b, d
                             (which must keep sweep 0's)              filters every entry.  0x00 hides it; a three-launch
                                                                      previous leaves its own pad0 there (the fill's bytes)
  MoveTableHdr.first_bad     plan (~0), lowered by finish             as above; window, move and place do nothing if it is set  a1 a2 a4, c
  MoveTableHdr.total         plan (0), finish always stores it        none (read behind finish's store)                          a, c
  MoveTableHdr.up            plan (0), finish always stores it        none (read behind finish's store); a stale 1 would walk    a3 a4, b
                                                                      a downward table backwards
  MoveTableHdr.pad0, pad1    never read                               --                                                         --
  blk records                plan stores each whole (thread 1023      none for k < n_blk; records past n_blk are never read:     a2, b
                             of every workgroup), MoveTableBlk.pad     4097 entries leave five, a 17-entry call reads one
                             included
  plan records               plan stores entry i < n whole; finish    none for i < n; a record past n is reached only through    a1, b
                             rewrites start                           a missing pad (next row)
  search levels and pad      finish: every entry's key at every       0x00 and a larger previous table: a stale key <= g in the  a1, b
                             level <= top, then ~0 up to the next      last line of 16 sends the descent past entry n - 1, to a
                             multiple of 16 keys, top and sizes        stale plan record: chunks are lost.  0xFF hides it.  n =
                             from n                                    1, 17, 257, 1025, 4097 have a ragged last line at level 0,
                                                                      17 and 257 at level 1, 4097 at levels 1, 2 and 3
  edge records (rekey kinds) plan stores entry i < n whole            none                                                       a, b
  move flags                 plan clears all `cap` of them            any nonzero flag: a store goes out before the chunk whose  a2 a3 a4, b, d
                             (cap = total_bytes / 64 KiB + 2 n,        source it overwrites was loaded -- the tables here lay
                             not from the table)                       destinations over other entries' sources.  0x00 hides it;
                                                                      a previous moving call leaves every flag of its chunks up
  windows                    window launch, chunk g < total           none: read for g < total only                              a, b
  scratch                    finish, the head_n / tail_n bytes        none: place reads exactly those bytes                      a, b
  verify summary line        plan: mismatches 0, first_bad_entry ~0,  mismatches: any nonzero fill and a previous verifying      a (the two
                             entries n, reserved 0                    call; first_bad_entry: 0x00 and a previous call; entries:  verifying
                                                                      everything but the same n                                  kinds), b, d
  digest accumulators        the records, in the caller's buffer,     the adapter fills the records with 0x5A before EVERY       every case of
                             not in W: finish stores each whole       call: a record that was only added to is wrong             a digesting
                             ("no memset node"), stream adds                                                                     kind
  single move: header,       hipMemsetAsync of header and flags       ticket, status word, flags as above                        a2 a3 a4, b
  status word, flags         (the whole header on the rekey route)
  bytes past workspace_bytes nothing may write them                   every fill: W outside the range is compared after every    every case
                                                                      call

(A stale move flag changes bytes only when workgroups race for it: the CPU stand-in walks the positions in order and cannot show one,
so that row is this module's alone; every other row's case also runs on the stand-in, tests/test_workspace_reuse_cpu.py.)"""
import numpy as np
import pytest

import workspace_reuse as R
from hip_rt import Graph, Stream

pytestmark = pytest.mark.gpu

# the case count is a condition: all ten kinds under all four fills (0x00 first), all 100 ordered pairs in both size orders, every kind
# at the odd alignment -- asserted when the module is collected, and every one of them is a test or a loop turn below, none skipped
assert [f for f, _ in R.FILL_CASES[::10]] == ["zero", "leftover", "ones", "random"] and len(R.FILL_CASES) == 40
assert sorted(R.FILL_CASES) == sorted((f, k) for f in R.FILLS for k in R.KINDS) and len(R.KINDS) == 10
assert len(R.PAIR_CASES) == 200 and len(set(R.PAIR_CASES)) == 200 and {(a, b) for _, _, a, b in R.PAIR_CASES} == {(4097, 17), (17, 4097)}
assert all(sum(1 for p, _, _, _ in R.PAIR_CASES if p == prev) == 20 for prev in R.KINDS)
assert sorted(R.ALIGN_CASES) == sorted(R.KINDS)
GRAPH_N = 257


@pytest.fixture(scope="module")
def gpu(modgpu):
    assert modgpu.device_count() >= 1, "no MI355X visible: the GPU tests cannot run"
    assert modgpu.gpu_required(), "conftest must have set MODGPU_REQUIRE_GPU=1 before the library was loaded"
    return modgpu


@pytest.fixture(scope="module")
def K(oracle):
    return R.Keystreams(oracle)


@pytest.fixture(scope="module")
def rig(gpu, K):
    """one W for the whole module: what a test finds in it is what the test before left"""
    with R.rig(gpu, K, R.all_cases(), sites=3) as r:
        yield r
        assert gpu.path_stats()["scalar_calls"] == 0


@pytest.mark.parametrize("fill,kind", R.FILL_CASES, ids=[f"{f}-{k}" for f, k in R.FILL_CASES])
def test_fill(rig, fill, kind):
    """a: the kind at seven table lengths on every side, W pre-filled.  The 0xFF and random fills fail, not skip, for a kind that has
    not passed the 0x00 and leftover fills in this session: garbage read as a plan record would be a wild pointer"""
    blocked = R.fill_blocked(fill, kind)
    if blocked:
        pytest.fail(blocked)
    R.run_fill(rig, fill, kind)
    assert (fill, kind) in R.PASSED


@pytest.mark.parametrize("prev", R.KINDS)
def test_every_next_kind_after(rig, prev):
    """b: `prev` at 4097 entries then each of the ten kinds at 17, `prev` at 17 then each at 4097; W is not touched in between"""
    nexts = [(q, a, b) for p, q, a, b in R.PAIR_CASES if p == prev]
    assert len(nexts) == 20
    for nxt, a, b in nexts:
        R.run_pairs(rig, prev, nexts=(nxt,), orders=((a, b),))


@pytest.mark.parametrize("prev", R.REFUSAL_PREVIOUS)
def test_refusals_across_kinds(rig, prev):
    """c: a refused call of one header family, then a clean call of every other kind: status clean, outputs right; and a clean call,
    then a refused one of every other kind: the status names entry 123, arena, records and guards byte for byte what they were"""
    R.run_refusals(rig, prev)


def test_verify_summary_is_the_last_calls(rig):
    """d: entries, mismatches and first_bad_entry of a 17-entry verifying call behind a 4097-entry one with planted mismatches"""
    R.run_verify_summaries(rig)


def test_move_table_status_after_a_clean_call_on_each_fill(rig):
    R.run_move_statuses(rig)


def test_digest_check_reads_the_producers_header(rig):
    """d: behind a refused call of ANOTHER kind a clean producer's records are compared (refused clear, the bad count and bitmap
    right); a refused producer makes the check say so and compare nothing"""
    R.run_checks(rig)


@pytest.mark.parametrize("kind", R.ALIGN_CASES)
def test_workspace_8_modulo_64(rig, kind):
    """e: the contract's "8-byte aligned" and nothing more"""
    R.run_aligned(rig, kind)


def test_three_kinds_in_one_captured_chain(gpu, rig, K):
    """f: cycle_digest_table, rekey_move_table and verify_table on one stream and one W, captured as one linear chain and replayed
    twice, one entry of each table rewritten in between; each call's workspace is its own size of the same W"""
    kinds = ("cycle_digest_table", "rekey_move_table", "verify_table")
    st = Stream()
    try:
        cases = [R.Case(k, GRAPH_N) for k in kinds]
        for site, case in enumerate(cases):
            rig.lay(case, site)
        with Graph.capture(st) as g:
            for site, case in enumerate(cases):
                rig.call(case, 0, site, stream=st.handle)
        for variant in (0, 1):
            cases = [R.Case(k, GRAPH_N, variant=variant) for k in kinds]
            for site, case in enumerate(cases):
                assert variant == 0 or not np.array_equal(R.entries(gpu, case, 0), R.entries(gpu, R.Case(case.kind, GRAPH_N), 0))
                rig.lay(case, site)
            before, room = rig.mirror, max(R.need(gpu, c) for c in cases)
            g.launch(st)
            st.sync()
            for site, case in enumerate(cases):
                last = site == len(cases) - 1
                want = {k: v for k, v in R.model(case, K).items() if k != "launches" and (last or k in ("arena", "record_guards", "records"))}
                R.compare(rig.gather(case, 0, site, status=last), want, ("replay", variant, case))
            rig.mirror = rig.W.download()
            a, b = rig.inner, rig.inner + room
            assert np.array_equal(rig.mirror[:a], before[:a]) and np.array_equal(rig.mirror[b:], before[b:]), ("W outside the workspaces", variant)
        g.destroy()
    finally:
        st.destroy()
