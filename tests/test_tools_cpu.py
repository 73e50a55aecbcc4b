"""CPU checks of the measurement tooling that turns profiler output into the figures DESIGN.md quotes (no GPU, no profiler needed:
synthetic inputs in the formats `bin/modbench --route` and `rocprofv3 --kernel-trace --output-format csv` write)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADER = ('"Kind","Agent_Id","Queue_Id","Stream_Id","Thread_Id","Dispatch_Id","Kernel_Id","Kernel_Name","Correlation_Id","Start_Timestamp","End_Timestamp",'
          '"LDS_Block_Size","Scratch_Size","VGPR_Count","Accum_VGPR_Count","SGPR_Count","Workgroup_Size_X","Workgroup_Size_Y","Workgroup_Size_Z","Grid_Size_X","Grid_Size_Y","Grid_Size_Z"')


def row(queue, tid, disp, start, end, grid=32 * 256):
    return f'"KERNEL_DISPATCH","Agent 2",{queue},{queue},{tid},{disp},11,"void modgpu_cycle_kernel<1, 256, 1, false>(CycleArgs)",{disp},{start},{end},0,0,43,0,48,256,1,1,{grid},1,1'


def test_pcie_trace_join_by_thread_and_order(tmp_path):
    """tools/summarize_pcie_trace.py: a thread's launches (the library's host trace) and its dispatches (the profiler's kernel trace) are in
    the same order; the join gives every kernel its bytes and call, and from that bytes / duration, the busy share of a call's wall
    clock, how many kernels ran at once and the gaps on a queue."""
    log = tmp_path / "route.log"
    # two calls (call 0 is the untimed warm-up: no wall time), two pipeline threads, pieces of 1 and 4 MiB
    log.write_text("\n".join([
        "route staged  bytes 10485760  reps 1",
        "hashes kernel ddcc feed ffee",
        "call 1 wall_us 400.0",
        "callbegin 0 t_us 0.0", "launch tid 101 call 0 pipe 0 piece 0 bytes 1048576 t_us 10.0", "launch tid 102 call 0 pipe 1 piece 1 bytes 4194304 t_us 12.0", "callend 0 t_us 300.0",
        "callbegin 1 t_us 1000.0", "launch tid 101 call 1 pipe 0 piece 0 bytes 1048576 t_us 1010.0", "launch tid 102 call 1 pipe 1 piece 1 bytes 4194304 t_us 1012.0",
        "launch tid 101 call 1 pipe 0 piece 2 bytes 4194304 t_us 1100.0", "callend 1 t_us 1400.0", ""]))
    d = tmp_path / "prof" / "host"
    d.mkdir(parents=True)
    us = 1000
    (d / "1_kernel_trace.csv").write_text("\n".join([HEADER,
        '"KERNEL_DISPATCH","Agent 2",1,1,101,1,9,"__amd_rocclr_fillBufferAligned",1,1,2,0,0,8,0,48,256,1,1,1024,1,1',
        row(1, 101, 2, 5000 * us, 5040 * us), row(2, 102, 3, 5010 * us, 5110 * us),                      # call 0
        row(1, 101, 4, 9000 * us, 9050 * us), row(2, 102, 5, 9020 * us, 9220 * us), row(1, 101, 6, 9100 * us, 9300 * us), ""]))  # call 1
    # what tools/ubench_pcie_ceiling prints last, from the same run: the figures the roofline is priced against
    ceil = tmp_path / "ceiling.txt"
    ceil.write_text('== table\nCEILING {"MiB": 1024, "peak_link": 64.0, "dma_h2d": 55.0, "dma_d2h": 56.0, "dma_duplex_per_direction": 47.0, '
                    '"product_pinned_route_in_place": 50.4, "kernel_source_hash": "aa", "feed_kernel_source_hash": "bb"}\n')
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "summarize_pcie_trace.py"), str(log), str(tmp_path / "prof"), "--ceilings", str(ceil)],
                       capture_output=True, text=True, check=True)
    out = json.loads(r.stdout)
    assert out["launches_listed"] == 5 and out["dispatches_traced"] == 5 and out["unmatched"] == 0
    c1 = [c for c in out["per_call"] if c["call"] == 1][0]
    assert c1["kernels"] == 3 and c1["bytes"] == 9 << 20 and c1["wall_us"] == 400.0
    assert c1["kernel_window_us"] == 300.0 and c1["busy_us"] == 300.0  # [9000, 9300] us, covered without a hole
    assert abs(c1["busy_frac_of_wall"] - 0.75) < 1e-9
    assert abs(c1["mean_kernels_at_once_while_busy"] - (50 + 200 + 200) / 300) < 0.01
    assert c1["gaps_on_a_queue_us"]["n"] == 1 and c1["gaps_on_a_queue_us"]["median"] == 50.0  # queue 1: 9050 -> 9100
    by = {k["bytes"]: k for k in out["per_kernel_by_bytes"]}   # timed calls only: call 1
    assert by[1 << 20]["n"] == 1 and by[1 << 20]["median_us"] == 50.0 and by[4 << 20]["n"] == 2 and by[4 << 20]["median_us"] == 200.0
    assert abs(by[4 << 20]["payload_GBps_at_median"] - (4 << 20) / 200e-6 / 1e9) < 0.01
    # the peak is the link on paper, with the DMA engines' figures of the same run beside it -- nothing the library's own kernel produced
    rf = out["roofline_pcie"]
    ach = (9 << 20) / 400e-6 / 1e9
    assert rf["bound"] == "pcie" and rf["peak"] == rf["peak_link"] == 64.0 and abs(rf["achieved"] - ach) < 0.01
    assert abs(rf["frac_of_link"] - ach / 64.0) < 1e-3 and rf["dma_one_way"] == 55.0 and rf["dma_duplex"] == 47.0
    assert abs(rf["frac_of_dma_one_way"] - ach / 55.0) < 1e-3 and abs(rf["frac_of_dma_duplex"] - ach / 47.0) < 1e-3
    assert rf["reference_only_one_kernel_in_place"] == 50.4 and rf["dispatches_per_timed_call"] == 3
    assert out["feed_kernel_source_hash"] == rf["feed_kernel_source_hash"] == "ffee" and out["kernel_source_hash"] == "ddcc"


def test_kernel_trace_summary_by_kernel_and_grid(tmp_path):
    p = tmp_path / "k_kernel_trace.csv"
    p.write_text("\n".join([HEADER, row(1, 7, 1, 0, 8_000_000, grid=256 * 256), row(1, 7, 2, 9_000_000, 17_200_000, grid=256 * 256), row(2, 8, 3, 100, 5600, grid=2048 * 256), ""]))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "summarize_kernel_trace.py"), str(p)], capture_output=True, text=True, check=True)
    out = json.loads(r.stdout)
    assert out["dispatches"] == 3
    big = out["by_kernel_and_grid"][0]
    assert big["workgroups"] == 256 and big["dispatches"] == 2 and big["median_us"] == 8100.0 and big["total_us"] == 16200.0
    assert out["by_kernel_and_grid"][1]["workgroups"] == 2048 and out["by_kernel_and_grid"][1]["median_us"] == 5.5


# ---- tools/bench_common.py: the harness of the fourteen event-timed bench tools

TOOLS = os.path.join(ROOT, "tools")
# tool -> (factor of the rate, its key): what each tool passes to bench_common.stats
BENCH_RATES = {"bench_cycle_to": (2, "TBps_2n"), "bench_rekey": (2, "TBps_2n"), "bench_table": (2, "TBps_2n"), "bench_rekey_table": (2, "TBps_2n"),
               "bench_verify": (2, "TBps_2n"), "bench_verify_table": (2, "TBps_2n"), "bench_keep": (2, "TBps_2n"), "bench_verify_rekey": (2, "TBps_2n"),
               "bench_verify_rekey_table": (2, "TBps_2n"), "bench_rekey_move": (1, "TBps"), "bench_rekey_move_table": (1, "TBps"),
               "bench_digest": (1, "TBps_n"), "bench_digest_table": (1, "TBps"), "bench_cycle_digest_table": (1, "TBps")}


def _bench_common():
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    import bench_common
    return bench_common


def _profiles():
    """(tool name, document) of every committed profile one of the fourteen tools wrote"""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*.json"))):
        with open(path) as f:
            doc = json.load(f)
        tool = os.path.basename(str(doc.get("tool", "")) if isinstance(doc, dict) else "").replace(".py", "")
        if tool in BENCH_RATES:
            yield tool, doc


def test_bench_common_import_has_no_side_effects():
    """Importing the harness writes no environment variable and loads neither the HIP runtime nor libmodgpu: setup() does, when a tool
    asks for it.  In a child process, so that nothing this test process loaded counts."""
    code = "\n".join([
        "import os, sys",
        "before = dict(os.environ)",
        f"sys.path.insert(0, {TOOLS!r})",
        "import bench_common",
        "assert dict(os.environ) == before, 'the import changed os.environ'",
        "assert 'modulate_amd' not in sys.modules and 'hip_rt' not in sys.modules, sorted(m for m in sys.modules if 'mod' in m or 'hip' in m)",
        "import modulate_amd.capi as capi",
        "import hip_rt",
        "assert capi._libs == {} and hip_rt._hip is None",
        "maps = open('/proc/self/maps').read()",
        "assert 'libamdhip64' not in maps and 'libmodgpu' not in maps",
        "assert 'MODGPU_REQUIRE_GPU' not in os.environ or before.get('MODGPU_REQUIRE_GPU') == os.environ['MODGPU_REQUIRE_GPU']",
        "print('clean')"])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "clean", r.stderr


def test_bench_stats_reproduces_the_recorded_rates():
    """Every (row, variant) of the committed profiles: the rate of the recorded bytes at the recorded median, with the tool's factor,
    is the recorded rate -- within rate x 5.1e-6 / median_ms + 5.1e-5, the worst case of the recorded median's rounding to 5 places
    plus the recorded rate's own rounding to 4 (derived, not measured) -- and bench_common.stats gives that rate, rounded."""
    H = _bench_common()
    pairs = 0

    def variants(node, key):
        if isinstance(node, dict):
            if "median_ms" in node and key in node:
                yield node
            else:
                for child in node.values():
                    yield from variants(child, key)

    def rows(node):
        if isinstance(node, dict):
            if "bytes" in node:
                yield node
            else:
                for child in node.values():
                    yield from rows(child)

    for tool, doc in _profiles():
        factor, key = BENCH_RATES[tool]
        for row in rows(doc):
            for v in variants(row, key):
                rate = factor * row["bytes"] / (v["median_ms"] * 1e-3) / 1e12
                assert abs(rate - v[key]) <= v[key] * 5.1e-6 / v["median_ms"] + 5.1e-5, (tool, row["bytes"], v)
                assert H.stats([v["median_ms"]], row["bytes"], factor, key)[key] == round(rate, 4)  # stats is that formula, rounded
                pairs += 1
    assert pairs >= 300, pairs


def test_bench_stats_on_fixed_times():
    H = _bench_common()
    assert H.stats([3.0, 1.0, 2.0], 1 << 30, 2, "TBps_2n") == {"median_ms": 2.0, "min_ms": 1.0, "max_ms": 3.0, "TBps_2n": 1.0737}
    # an even count: the upper of the two middle times
    assert H.stats([4.0, 1.0, 0.123456789, 2.0], 10 ** 9, 1, "TBps") == {"median_ms": 2.0, "min_ms": 0.12346, "max_ms": 4.0, "TBps": 0.5}
    assert H.stats([0.02], 65536, 1, "TBps_n") == {"median_ms": 0.02, "min_ms": 0.02, "max_ms": 0.02, "TBps_n": 0.0033}
    row = {"base": {"median_ms": 3.0}, "table": {"median_ms": 1.5}, "table2": {"median_ms": 1.6}}
    H.add_speedups(row, ["table", "base"])
    assert row["table_speedup_over_base"] == 2.0 and H.aa_spread(row, "table") == 0.06667
    H.add_speedups(row, ["table2"])
    assert "table2_speedup_over_base" not in row


def test_bench_table_layouts_are_the_recorded_ones():
    """bench_common.table_layout against tests/bench_layouts.json -- the SHA-256 of every array each tool's own layout() returned
    before the harness took them over, with its entry count and byte total -- and against the entries and bytes of the committed
    profiles, which were taken on those tables."""
    import hashlib
    H = _bench_common()
    with open(os.path.join(ROOT, "tests", "bench_layouts.json")) as f:
        want = json.load(f)
    assert sorted(want) == sorted(t + "/" + s for t, shapes in H.LAYOUT_SHAPES.items() for s in shapes)
    for name, w in want.items():
        tool, shape = name.split("/")
        got = H.table_layout(tool, shape)
        parts = [hashlib.sha256(x.tobytes()).hexdigest() + ":" + str(x.dtype) if hasattr(x, "tobytes") else int(x) for x in got]
        assert parts == w["parts"], name
        assert (int(got[0].size), int(got[0].sum())) == (w["entries"], w["bytes"]), name
    assert (want["table/config4"]["entries"], want["table/config4"]["bytes"]) == (100000, 3278797672)
    assert (want["digest_table/16kx64k"]["entries"], want["digest_table/16kx64k"]["bytes"]) == (16384, 1073741824)
    seen = 0
    for tool, doc in _profiles():
        layout = tool[len("bench_"):]
        for shape, row in doc.get("shapes", {}).items():
            if layout in H.LAYOUT_SHAPES and shape in H.LAYOUT_SHAPES[layout]:
                assert (row["entries"], row["bytes"]) == (want[layout + "/" + shape]["entries"], want[layout + "/" + shape]["bytes"]), (tool, shape)
                seen += 1
    assert seen >= 20, seen
    for tool in H.LAYOUT_SHAPES:
        for shape in ("nonsense",) + tuple(s for s in H.SINGLE_ENTRY if s not in H.LAYOUT_SHAPES[tool]):
            try:
                H.table_layout(tool, shape)
            except ValueError:
                continue
            raise AssertionError((tool, shape))
