"""What the HOST side of the C ABI promises, pinned against a recording of the build before the host layer was shared
(tests/golden/host_contract_parent.json): the status code and the exact last-error text of every call the four handle types reject, the status
of every entry point on NULL and on a destroyed handle, and what pv_get_info reports for each kernel family -- kernel name, threads and LDS per
workgroup, and frames_per_chunk after a batch (the only place the chunking choice shows: split-invariance hides it from the bits tests).

A rejected call changes nothing: after each group of rejections the exported state is compared, bit for bit, with the state before it.

The CPU part needs no device: every create call in it is rejected on its arguments.  The fixture is recorded the way
tests/test_gpu_frame_bits.py records its own:
    PHAZE_LIB=<library of the build to pin> python tests/test_host_contract.py --record tests/golden/host_contract_parent.json
(on a machine without a device only the "cpu" section is rewritten).  Every call sequence runs on a fresh thread, so that the thread-local
create-error buffers start empty whatever ran before in the process."""
import ctypes as C
import json
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)                         # (run as a script: --record)
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_contract_parent.json")
TYPES = ("pv", "pv_stretch", "pv_resample", "pv_pitch")
FLAG_GENERIC, FLAG_WORKGROUP, FLAG_PERSISTENT = 1, 4, 32
FAMILY_CASES = [("1024_256", 1024, 256, 0), ("2048_128", 2048, 128, 0), ("4096_512", 4096, 512, 0), ("4096_512_workgroup", 4096, 512, FLAG_WORKGROUP),
                ("2048_128_generic", 2048, 128, FLAG_GENERIC), ("2048_128_workgroup", 2048, 128, FLAG_WORKGROUP)]
BATCHES = [(1, 1), (3, 7), (2, 200)]
RESIDENT_CASES = [("1024_256", 1024, 256), ("4096_512", 4096, 512)]


def _on_fresh_thread(fn, *args):
    box = {}

    def body():
        try:
            box["value"] = fn(*args)
        except BaseException as e:          # noqa: BLE001 -- handed to the caller's thread
            box["error"] = e
    t = threading.Thread(target=body)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


def _lib():
    from phaze_amd import capi
    return capi.load_library()


# ---------------------------------------------------------------- CPU part: the four create functions

def _cpu_cases():
    """(name, handle type, config or None, pass an out pointer)"""
    from phaze_amd import capi
    pv, st, rs, pt = capi.make_config, capi.make_stretch_config, capi.make_resample_config, capi.make_pitch_config

    def shrunk(cfg):
        cfg.struct_size -= 4
        return cfg
    return [
        ("pv/null_config", "pv", None, True), ("pv/null_out", "pv", pv(1024, 256), False), ("pv/struct_size", "pv", shrunk(pv(1024, 256)), True),
        ("pv/unknown_flags", "pv", pv(1024, 256, flags=1 << 20), True),
        ("pv/fft_size_1000", "pv", pv(1000, 250), True), ("pv/fft_size_1", "pv", pv(1, 1), True), ("pv/fft_size_0", "pv", pv(0, 128), True),
        ("pv/fft_size_too_large", "pv", pv(1 << 21, 1 << 10), True),
        ("pv/hop_0", "pv", pv(1024, 0), True), ("pv/hop_negative", "pv", pv(1024, -256), True), ("pv/hop_not_a_divisor", "pv", pv(1024, 300), True),
        ("pv/hop_1", "pv", pv(1024, 1), True),
        ("pv/generic_kernel_lds_8192_256", "pv", pv(8192, 256, flags=FLAG_GENERIC), True),
        ("stretch/null_config", "pv_stretch", None, True), ("stretch/null_out", "pv_stretch", st(256, 64, 64), False),
        ("stretch/struct_size", "pv_stretch", shrunk(st(256, 64, 64)), True), ("stretch/unknown_flags", "pv_stretch", st(256, 64, 64, flags=1), True),
        ("stretch/fft_size_1000", "pv_stretch", st(1000, 250, 250), True),
        ("stretch/fft_size_128", "pv_stretch", st(128, 32, 32), True), ("stretch/fft_size_16384", "pv_stretch", st(16384, 1024, 1024), True),
        ("stretch/analysis_hop_0", "pv_stretch", st(256, 0, 64), True), ("stretch/analysis_hop_above_n", "pv_stretch", st(256, 257, 64), True),
        ("stretch/synthesis_hop_0", "pv_stretch", st(256, 64, 0), True), ("stretch/synthesis_hop_above_half", "pv_stretch", st(256, 64, 129), True),
        ("stretch/too_many_channels", "pv_stretch", st(256, 64, 64, max_channels=65536), True),
        ("resample/null_config", "pv_resample", None, True), ("resample/null_out", "pv_resample", rs(3, 2), False),
        ("resample/struct_size", "pv_resample", shrunk(rs(3, 2)), True), ("resample/unknown_flags", "pv_resample", rs(3, 2, flags=2), True),
        ("resample/up_0", "pv_resample", rs(0, 2), True), ("resample/down_negative", "pv_resample", rs(3, -1), True),
        ("resample/ratio_9", "pv_resample", rs(9, 1), True), ("resample/ratio_1_9", "pv_resample", rs(1, 9), True),
        ("resample/term_8193", "pv_resample", rs(8193, 8192), True), ("resample/too_many_channels", "pv_resample", rs(3, 2, max_channels=65536), True),
        ("pitch/null_config", "pv_pitch", None, True), ("pitch/null_out", "pv_pitch", pt(256, 64, 96), False),
        ("pitch/struct_size", "pv_pitch", shrunk(pt(256, 64, 96)), True), ("pitch/unknown_flags", "pv_pitch", pt(256, 64, 96, flags=4), True),
        ("pitch/up_negative", "pv_pitch", pt(256, 64, 96, up=-1, down=1), True), ("pitch/ratio_9", "pv_pitch", pt(256, 64, 96, up=9, down=1), True),
        ("pitch/up_only", "pv_pitch", pt(256, 64, 96, up=2, down=0), True), ("pitch/hops_ratio_1_16", "pv_pitch", pt(2048, 64, 1024), True),
        ("pitch/fft_size_1000", "pv_pitch", pt(1000, 250, 250), True), ("pitch/fft_size_128", "pv_pitch", pt(128, 32, 32), True),
        ("pitch/analysis_hop_above_n", "pv_pitch", pt(256, 257, 64, up=1, down=1), True),
        ("pitch/synthesis_hop_above_half", "pv_pitch", pt(256, 64, 129, up=1, down=1), True),
        ("pitch/too_many_channels", "pv_pitch", pt(256, 64, 96, max_channels=65536), True),
    ]


CPU_NAMES = [c[0] for c in _cpu_cases()]


def run_cpu():
    """name -> {status, errors: the four create-error buffers after the call, others_unchanged}.  pv_pitch_create reads the create buffers of
    the two inner types, so it may write them; every other create leaves the other three buffers alone."""
    L = _lib()

    def errors():
        return {t: getattr(L, t + "_last_error")(None).decode() for t in TYPES}
    out = {}
    for name, typ, cfg, want_out in _cpu_cases():
        before = errors()
        h = C.c_void_p()
        rc = getattr(L, typ + "_create")(C.byref(cfg) if cfg is not None else None, C.byref(h) if want_out else None)
        assert not h.value, f"{name}: the call was meant to be rejected"
        after = errors()
        may_change = {typ} | ({"pv_stretch", "pv_resample"} if typ == "pv_pitch" else set())
        out[name] = {"status": rc, "errors": after, "others_unchanged": all(after[t] == before[t] for t in TYPES if t not in may_change)}
    return out


# ---------------------------------------------------------------- GPU part

def _null_args(fn):
    """Arguments behind the handle for a call that must return on the handle check alone."""
    return [0.0 if t is C.c_float else 0 if t in (C.c_int, C.c_int32, C.c_int64, C.c_size_t) else None for t in fn.argtypes[1:]]


DEAD_CALLS = {
    "pv": ["pv_get_info", "pv_reset", "pv_reset_channels", "pv_reset_channels_part", "pv_get_time_cursor", "pv_set_time_cursor", "pv_process",
           "pv_process_begin", "pv_process_end", "pv_process_batch", "pv_process_batch_device", "pv_set_stream", "pv_synchronize", "pv_debug_frame",
           "pv_export_state", "pv_import_state", "pv_forward_stats"],
    "pv_stretch": ["pv_stretch_reset", "pv_link_channels", "pv_stretch_set_stream", "pv_stretch_synchronize", "pv_stretch_process",
                   "pv_stretch_process_device", "pv_tempo_process", "pv_tempo_process_device", "pv_transient_process", "pv_transient_process_device",
                   "pv_onset_strength", "pv_onset_strength_device", "pv_transient_chain_layout", "pv_onset_chain_layout", "pv_stretch_export_state",
                   "pv_stretch_import_state"],
    "pv_resample": ["pv_resample_reset", "pv_resample_set_stream", "pv_resample_synchronize", "pv_resample_process", "pv_resample_process_device",
                    "pv_resample_out_count", "pv_resample_export_state", "pv_resample_import_state"],
    "pv_pitch": ["pv_pitch_reset", "pv_pitch_set_stream", "pv_pitch_synchronize", "pv_pitch_process", "pv_pitch_process_device", "pv_pitch_stretch",
                 "pv_pitch_resampler"],
}


def run_gpu():
    """{"errors": name -> [status, last error of the handle], "unchanged": group -> the state after the group equals the state before,
    "dead": name -> status, "families": ...}"""
    import torch
    from phaze_amd import capi
    L = _lib()
    fp, ip, bp, up = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    res = {"errors": {}, "unchanged": {}, "dead": {}, "families": {}, "resident": {}}

    def f32(a):
        return a.ctypes.data_as(fp)

    def i32(a):
        return a.ctypes.data_as(ip)

    def u8(a):
        return a.ctypes.data_as(bp)

    def signal(nch, n, seed):
        t = np.arange(n, dtype=np.float64)
        return np.stack([0.4 * np.sin(0.031 * (c + 1 + seed) * t) + 0.2 * np.cos(0.0071 * t * (seed + 2)) for c in range(nch)]).astype(np.float32)

    def create(typ, cfg):
        h = C.c_void_p()
        rc = getattr(L, typ + "_create")(C.byref(cfg), C.byref(h))
        assert rc == 0, getattr(L, typ + "_last_error")(None).decode()
        return h

    def group(prefix, last_error, h, state, calls):
        """Issues the calls (name, thunk) and records [status, last error]; none may succeed, and the state must not move."""
        before = state()
        for name, thunk in calls:
            rc = thunk()
            assert rc != 0, f"{prefix}/{name}: the call was meant to be rejected"
            res["errors"][f"{prefix}/{name}"] = [rc, last_error(h).decode()]
        res["unchanged"][prefix] = state() == before

    # ---- pv_handle: 1024 / 256, two channels, four hops
    N, hop = 1024, 256
    h = create("pv", capi.make_config(N, hop, 2, 4))
    x, y, pitch = signal(3, 4 * hop, 0), np.zeros((3, 4 * hop), np.float32), np.full(4, 1.25, np.float32)
    d_x, d_y, d_p = torch.from_numpy(x).cuda(), torch.zeros(3, 4 * hop, device="cuda"), torch.full((4,), 1.25, device="cuda")
    torch.cuda.synchronize()
    ins = (fp * 3)(*[f32(x[c]) for c in range(3)])
    outs = (fp * 3)(*[f32(y[c]) for c in range(3)])

    def pv_state():
        parts = []
        for ch in range(2):
            hist, acc, tc = np.zeros(N - hop, np.float32), np.zeros(N - hop, np.float32), C.c_int64()
            assert L.pv_export_state(h, ch, f32(hist), f32(acc), C.byref(tc)) == 0
            parts += [hist.tobytes(), acc.tobytes(), tc.value]
        assert any(np.frombuffer(parts[0], np.float32)) and any(np.frombuffer(parts[1], np.float32))
        return parts
    assert L.pv_process_batch(h, f32(x), f32(y), 2, 4, 4 * hop, f32(pitch), 0, 1) == 0, L.pv_last_error(h)
    group("pv_process", L.pv_last_error, h, pv_state, [
        ("too_many_channels", lambda: L.pv_process(h, ins, outs, 3, hop, 1.0)),
        ("negative_channels", lambda: L.pv_process(h, ins, outs, -1, hop, 1.0)),
        ("null_out", lambda: L.pv_process(h, ins, None, 1, hop, 1.0)),
        ("nsamples_not_hop", lambda: L.pv_process(h, ins, outs, 2, 100, 1.0)),
        ("begin_too_many_channels", lambda: L.pv_process_begin(h, ins, 3, hop, 1.0)),
        ("end_nothing_pending", lambda: L.pv_process_end(h, outs)),
    ])
    group("pv_batch", L.pv_last_error, h, pv_state, [
        ("null_in", lambda: L.pv_process_batch(h, None, f32(y), 2, 4, 4 * hop, f32(pitch), 0, 1)),
        ("null_out", lambda: L.pv_process_batch(h, f32(x), None, 2, 4, 4 * hop, f32(pitch), 0, 1)),
        ("null_pitch", lambda: L.pv_process_batch(h, f32(x), f32(y), 2, 4, 4 * hop, None, 0, 1)),
        ("no_channels", lambda: L.pv_process_batch(h, f32(x), f32(y), 0, 4, 4 * hop, f32(pitch), 0, 1)),
        ("no_hops", lambda: L.pv_process_batch(h, f32(x), f32(y), 2, 0, 4 * hop, f32(pitch), 0, 1)),
        ("too_many_channels", lambda: L.pv_process_batch(h, f32(x), f32(y), 3, 4, 4 * hop, f32(pitch), 0, 1)),
        ("too_many_hops", lambda: L.pv_process_batch(h, f32(x), f32(y), 2, 5, 5 * hop, f32(pitch), 0, 1)),
        ("short_ch_stride", lambda: L.pv_process_batch(h, f32(x), f32(y), 2, 2, 100, f32(pitch), 0, 1)),
        ("negative_pitch_stride", lambda: L.pv_process_batch(h, f32(x), f32(y), 2, 2, 4 * hop, f32(pitch), -1, 1)),
        ("negative_channels_per_stream", lambda: L.pv_process_batch(h, f32(x), f32(y), 2, 2, 4 * hop, f32(pitch), 0, -1)),
        ("short_pitch_stride", lambda: L.pv_process_batch(h, f32(x), f32(y), 2, 2, 4 * hop, f32(pitch), 1, 1)),
    ])
    dx, dy, dp = d_x.data_ptr(), d_y.data_ptr(), d_p.data_ptr()
    group("pv_batch_device", L.pv_last_error, h, pv_state, [
        ("null_in", lambda: L.pv_process_batch_device(h, None, dy, 2, 4, 4 * hop, dp, 0, 1)),
        ("null_pitch", lambda: L.pv_process_batch_device(h, dx, dy, 2, 4, 4 * hop, None, 0, 1)),
        ("no_hops", lambda: L.pv_process_batch_device(h, dx, dy, 2, 0, 4 * hop, dp, 0, 1)),
        ("too_many_channels", lambda: L.pv_process_batch_device(h, dx, dy, 3, 4, 4 * hop, dp, 0, 1)),
        ("short_ch_stride", lambda: L.pv_process_batch_device(h, dx, dy, 2, 2, 100, dp, 0, 1)),
        ("short_pitch_stride", lambda: L.pv_process_batch_device(h, dx, dy, 2, 2, 4 * hop, dp, 1, 1)),
        ("negative_pitch_stride", lambda: L.pv_process_batch_device(h, dx, dy, 2, 2, 4 * hop, dp, -1, 1)),
        ("negative_channels_per_stream", lambda: L.pv_process_batch_device(h, dx, dy, 2, 2, 4 * hop, dp, 0, -1)),
    ])
    st_buf = np.zeros(N - hop, np.float32)
    group("pv_state", L.pv_last_error, h, pv_state, [
        ("cursor_not_a_multiple_of_hop", lambda: L.pv_set_time_cursor(h, 100)),
        ("cursor_negative", lambda: L.pv_set_time_cursor(h, -hop)),
        ("export_channel_out_of_range", lambda: L.pv_export_state(h, 2, f32(st_buf), None, None)),
        ("import_channel_out_of_range", lambda: L.pv_import_state(h, 2, f32(st_buf), None, -1)),
        ("import_channel_negative", lambda: L.pv_import_state(h, -1, f32(st_buf), None, -1)),
        ("import_cursor_not_a_multiple_of_hop", lambda: L.pv_import_state(h, 0, None, None, 100)),
        ("reset_part_no_parts", lambda: L.pv_reset_channels_part(h, 0, 1, 0)),
        ("reset_part_unknown_part", lambda: L.pv_reset_channels_part(h, 0, 1, 4)),
        ("reset_part_negative_first", lambda: L.pv_reset_channels_part(h, -1, 1, 3)),
        ("reset_part_range_too_long", lambda: L.pv_reset_channels_part(h, 1, 2, 3)),
        ("reset_part_negative_count", lambda: L.pv_reset_channels_part(h, 0, -1, 3)),
        ("reset_channels_range_too_long", lambda: L.pv_reset_channels(h, 1, 2)),
        ("debug_frame_channel_out_of_range", lambda: L.pv_debug_frame(h, 2, f32(x[0]), 1.0, None, None, None, None)),
        ("debug_frame_null_block", lambda: L.pv_debug_frame(h, 0, None, 1.0, None, None, None, None)),
        ("get_info_null", lambda: L.pv_get_info(h, None)),
        ("get_time_cursor_null", lambda: L.pv_get_time_cursor(h, None)),
    ])

    def quantum(pending_calls):
        """One streaming quantum from a reset handle, with the calls a pending quantum rejects issued between its begin and its end."""
        y[:] = 0
        assert L.pv_reset(h) == 0
        assert L.pv_process_begin(h, ins, 2, hop, 1.25) == 0, L.pv_last_error(h)
        for name, thunk in pending_calls:
            rc = thunk()
            assert rc != 0, f"pv_pending/{name}: the call was meant to be rejected"
            res["errors"][f"pv_pending/{name}"] = [rc, L.pv_last_error(h).decode()]
        assert L.pv_process_end(h, outs) == 0, L.pv_last_error(h)
        return pv_state() + [y[:2].tobytes()]
    y2 = np.zeros((2, 4 * hop), np.float32)
    with_rejections = quantum([
        ("batch", lambda: L.pv_process_batch(h, f32(x), f32(y2), 2, 4, 4 * hop, f32(pitch), 0, 1)),
        ("batch_device", lambda: L.pv_process_batch_device(h, dx, dy, 2, 4, 4 * hop, dp, 0, 1)),
        ("export_state", lambda: L.pv_export_state(h, 0, f32(st_buf), None, None)),
        ("import_state", lambda: L.pv_import_state(h, 0, f32(st_buf), None, -1)),
        ("begin", lambda: L.pv_process_begin(h, ins, 2, hop, 1.25)),
        ("process", lambda: L.pv_process(h, ins, (fp * 3)(*[f32(y2[c % 2]) for c in range(3)]), 2, hop, 1.25)),
    ])
    res["unchanged"]["pv_pending"] = with_rejections == quantum([]) and not y2.any()
    assert L.pv_destroy(h) == 0

    # ---- pv_stretch: 256 / 64 / 64, two channels
    N, ha, hs, H = 256, 64, 64, 129
    s = create("pv_stretch", capi.make_stretch_config(N, ha, hs, 2, 4))
    sx, sy = signal(3, 4 * N, 1), np.zeros((3, 4 * N), np.float32)
    d_sx, d_sy = torch.from_numpy(sx).cuda(), torch.zeros(3, 4 * N, device="cuda")
    d_counts = torch.zeros(64, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dsx, dsy, dc = d_sx.data_ptr(), d_sy.data_ptr(), d_counts.data_ptr()
    counts = np.zeros(64, np.int32)
    W = 4 * N                                        # the row pitch of sx / sy

    def stretch_state(handle=None, nh=N - ha, na=N - hs):
        parts = []
        for ch in range(2):
            hist, acc, phi, psi = np.zeros(nh, np.float32), np.zeros(na, np.float32), np.zeros(H, np.uint32), np.zeros(H, np.uint32)
            assert L.pv_stretch_export_state(handle or s, ch, f32(hist), f32(acc), phi.ctypes.data_as(up), psi.ctypes.data_as(up)) == 0
            parts += [hist.tobytes(), acc.tobytes(), phi.tobytes(), psi.tobytes()]
        assert any(np.frombuffer(parts[0], np.float32)) and any(np.frombuffer(parts[2], np.uint32))
        return parts
    assert L.pv_stretch_process(s, f32(sx), f32(sy), 2, 4, W, W) == 0, L.pv_stretch_last_error(s)
    hops = {k: np.array(v, np.int32) for k, v in {"ok": [64, 64], "below": [64, 32], "above": [300, 64], "rows": [[64, 128], [64, 64]],
                                                  "rows_differ": [[64, 64], [64, 128]]}.items()}
    flags = {k: np.array(v, np.uint8) for k, v in {"ok": [0, 1], "two": [0, 2], "rows_differ": [[0, 1], [0, 0]]}.items()}
    group("stretch_process", L.pv_stretch_last_error, s, stretch_state, [
        ("null_in", lambda: L.pv_stretch_process(s, None, f32(sy), 2, 2, W, W)),
        ("null_out", lambda: L.pv_stretch_process(s, f32(sx), None, 2, 2, W, W)),
        ("negative_channels", lambda: L.pv_stretch_process(s, f32(sx), f32(sy), -1, 2, W, W)),
        ("negative_frames", lambda: L.pv_stretch_process(s, f32(sx), f32(sy), 2, -1, W, W)),
        ("too_many_channels", lambda: L.pv_stretch_process(s, f32(sx), f32(sy), 3, 2, W, W)),
        ("short_in_stride", lambda: L.pv_stretch_process(s, f32(sx), f32(sy), 2, 2, 100, W)),
        ("short_out_stride", lambda: L.pv_stretch_process(s, f32(sx), f32(sy), 2, 2, W, 100)),
        ("device_null_in", lambda: L.pv_stretch_process_device(s, None, dsy, 2, 2, W, W)),
        ("device_too_many_channels", lambda: L.pv_stretch_process_device(s, dsx, dsy, 3, 2, W, W)),
        ("device_short_in_stride", lambda: L.pv_stretch_process_device(s, dsx, dsy, 2, 2, 100, W)),
    ])
    group("stretch_link", L.pv_stretch_last_error, s, stretch_state, [
        ("no_channels_per_group", lambda: L.pv_link_channels(s, 0)),
        ("more_than_max_channels", lambda: L.pv_link_channels(s, 3)),
    ])
    group("stretch_tempo", L.pv_stretch_last_error, s, stretch_state, [
        ("null_hops", lambda: L.pv_tempo_process(s, f32(sx), f32(sy), 2, 2, None, 0, W, W)),
        ("short_hop_stride", lambda: L.pv_tempo_process(s, f32(sx), f32(sy), 2, 2, i32(hops["rows"]), 1, W, W)),
        ("hop_below_analysis_hop", lambda: L.pv_tempo_process(s, f32(sx), f32(sy), 2, 2, i32(hops["below"]), 0, W, W)),
        ("hop_above_fft_size", lambda: L.pv_tempo_process(s, f32(sx), f32(sy), 2, 2, i32(hops["above"]), 0, W, W)),
        ("short_in_stride", lambda: L.pv_tempo_process(s, f32(sx), f32(sy), 2, 2, i32(hops["rows"]), 2, 100, W)),
        ("short_out_stride", lambda: L.pv_tempo_process(s, f32(sx), f32(sy), 2, 2, i32(hops["ok"]), 0, W, 100)),
        ("too_many_channels", lambda: L.pv_tempo_process(s, f32(sx), f32(sy), 3, 2, i32(hops["ok"]), 0, W, W)),
        ("device_hop_below_analysis_hop", lambda: L.pv_tempo_process_device(s, dsx, dsy, 2, 2, i32(hops["below"]), 0, W, W)),
        ("device_short_hop_stride", lambda: L.pv_tempo_process_device(s, dsx, dsy, 2, 2, i32(hops["rows"]), 1, W, W)),
        ("transient_short_reset_stride", lambda: L.pv_transient_process(s, f32(sx), f32(sy), 2, 2, i32(hops["ok"]), 0, u8(flags["rows_differ"]), 1, W, W)),
        ("transient_flag_2", lambda: L.pv_transient_process(s, f32(sx), f32(sy), 2, 2, i32(hops["ok"]), 0, u8(flags["two"]), 0, W, W)),
        ("transient_flat_hops_flag_2", lambda: L.pv_transient_process(s, f32(sx), f32(sy), 2, 2, None, 0, u8(flags["two"]), 0, W, W)),
        ("transient_hop_above_fft_size", lambda: L.pv_transient_process(s, f32(sx), f32(sy), 2, 2, i32(hops["above"]), 0, u8(flags["ok"]), 0, W, W)),
        ("transient_device_short_reset_stride",
         lambda: L.pv_transient_process_device(s, dsx, dsy, 2, 2, i32(hops["ok"]), 0, u8(flags["rows_differ"]), 1, W, W)),
        ("transient_device_null_out", lambda: L.pv_transient_process_device(s, dsx, None, 2, 2, i32(hops["ok"]), 0, u8(flags["ok"]), 0, W, W)),
    ])
    group("stretch_onset", L.pv_stretch_last_error, s, stretch_state, [
        ("null_counts", lambda: L.pv_onset_strength(s, f32(sx), 2, 2, W, None, 2)),
        ("short_in_stride", lambda: L.pv_onset_strength(s, f32(sx), 2, 2, 100, i32(counts), 2)),
        ("short_count_stride", lambda: L.pv_onset_strength(s, f32(sx), 2, 2, W, i32(counts), 1)),
        ("too_many_channels", lambda: L.pv_onset_strength(s, f32(sx), 3, 2, W, i32(counts), 2)),
        ("device_null_counts", lambda: L.pv_onset_strength_device(s, dsx, 2, 2, W, None, 2)),
        ("device_short_count_stride", lambda: L.pv_onset_strength_device(s, dsx, 2, 2, W, dc, 1)),
        ("export_channel_out_of_range", lambda: L.pv_stretch_export_state(s, 2, None, None, None, None)),
        ("import_channel_negative", lambda: L.pv_stretch_import_state(s, -1, None, None, None, None)),
        ("chain_layout_no_channels", lambda: L.pv_transient_chain_layout(s, 0, 4, None, None)),
        ("onset_chain_layout_no_frames", lambda: L.pv_onset_chain_layout(s, 2, 0, None)),
    ])
    assert L.pv_link_channels(s, 2) == 0                                     # (resets the state)
    assert L.pv_stretch_process(s, f32(sx), f32(sy), 2, 4, W, W) == 0, L.pv_stretch_last_error(s)
    group("stretch_linked", L.pv_stretch_last_error, s, stretch_state, [
        ("process_half_a_group", lambda: L.pv_stretch_process(s, f32(sx), f32(sy), 1, 2, W, W)),
        ("device_half_a_group", lambda: L.pv_stretch_process_device(s, dsx, dsy, 1, 2, W, W)),
        ("tempo_half_a_group", lambda: L.pv_tempo_process(s, f32(sx), f32(sy), 1, 2, i32(hops["ok"]), 0, W, W)),
        ("onset_half_a_group", lambda: L.pv_onset_strength(s, f32(sx), 1, 2, W, i32(counts), 2)),
        ("schedule_rows_differ", lambda: L.pv_tempo_process(s, f32(sx), f32(sy), 2, 2, i32(hops["rows_differ"]), 2, W, W)),
        ("reset_rows_differ", lambda: L.pv_transient_process(s, f32(sx), f32(sy), 2, 2, None, 0, u8(flags["rows_differ"]), 2, W, W)),
        ("chain_layout_half_a_group", lambda: L.pv_transient_chain_layout(s, 1, 4, None, None)),
    ])
    assert L.pv_stretch_destroy(s) == 0

    # ---- pv_resample: 3 / 2, two channels
    r = create("pv_resample", capi.make_resample_config(3, 2, 2, 64))
    T = 64                                           # taps per phase of 3 / 2
    rx, ry = signal(3, 200, 2), np.zeros((3, 400), np.float32)
    d_rx, d_ry = torch.from_numpy(rx).cuda(), torch.zeros(3, 400, device="cuda")
    torch.cuda.synchronize()
    drx, dry = d_rx.data_ptr(), d_ry.data_ptr()
    got = C.c_int64()

    def resample_state(handle=None, taps=T):
        parts = []
        for ch in range(2):
            hist, i, j = np.zeros(taps - 1, np.float32), C.c_int64(), C.c_int64()
            assert L.pv_resample_export_state(handle or r, ch, f32(hist), C.byref(i), C.byref(j)) == 0
            parts += [hist.tobytes(), i.value, j.value]
        assert any(np.frombuffer(parts[0], np.float32)) and parts[1] > 0
        return parts
    assert L.pv_resample_process(r, f32(rx), 2, 200, 200, f32(ry), 400, 400, C.byref(got)) == 0, L.pv_resample_last_error(r)
    group("resample", L.pv_resample_last_error, r, resample_state, [
        ("negative_channels", lambda: L.pv_resample_process(r, f32(rx), -1, 100, 200, f32(ry), 400, 400, None)),
        ("negative_samples", lambda: L.pv_resample_process(r, f32(rx), 2, -1, 200, f32(ry), 400, 400, None)),
        ("too_many_channels", lambda: L.pv_resample_process(r, f32(rx), 3, 100, 200, f32(ry), 400, 400, None)),
        ("null_in", lambda: L.pv_resample_process(r, None, 2, 100, 200, f32(ry), 400, 400, None)),
        ("null_out", lambda: L.pv_resample_process(r, f32(rx), 2, 100, 200, None, 400, 400, None)),
        ("out_capacity_too_small", lambda: L.pv_resample_process(r, f32(rx), 2, 100, 200, f32(ry), 400, 10, None)),
        ("short_in_stride", lambda: L.pv_resample_process(r, f32(rx), 2, 100, 10, f32(ry), 400, 400, None)),
        ("short_out_stride", lambda: L.pv_resample_process(r, f32(rx), 2, 100, 200, f32(ry), 10, 400, None)),
        ("device_null_in", lambda: L.pv_resample_process_device(r, None, 2, 100, 200, dry, 400, 400, None)),
        ("device_out_capacity_too_small", lambda: L.pv_resample_process_device(r, drx, 2, 100, 200, dry, 400, 10, None)),
        ("device_too_many_channels", lambda: L.pv_resample_process_device(r, drx, 3, 100, 200, dry, 400, 400, None)),
        ("out_count_negative", lambda: L.pv_resample_out_count(r, -1, C.byref(got))),
        ("out_count_null", lambda: L.pv_resample_out_count(r, 10, None)),
        ("export_channel_out_of_range", lambda: L.pv_resample_export_state(r, 2, None, None, None)),
        ("import_channel_out_of_range", lambda: L.pv_resample_import_state(r, 2, None, -1, -1)),
        ("import_counts_disagree", lambda: L.pv_resample_import_state(r, 0, None, 100, 0)),
    ])
    assert L.pv_resample_destroy(r) == 0

    # ---- pv_pitch: 256 / 64 / 96 (up / down = 64 / 96), two channels
    N, ha, hs = 256, 64, 96
    p = create("pv_pitch", capi.make_pitch_config(N, ha, hs, 0, 0, 2, 4))
    inner_s, inner_r = C.c_void_p(L.pv_pitch_stretch(p)), C.c_void_p(L.pv_pitch_resampler(p))
    px, py = signal(3, 4 * N, 3), np.zeros((3, 4 * N), np.float32)
    d_px, d_py = torch.from_numpy(px).cuda(), torch.zeros(3, 4 * N, device="cuda")
    torch.cuda.synchronize()
    dpx, dpy = d_px.data_ptr(), d_py.data_ptr()
    W = 4 * N

    def pitch_state():
        return stretch_state(inner_s, N - ha, N - hs) + resample_state(inner_r, 96)       # 2 / 3: W = 48, 96 taps per phase
    assert L.pv_pitch_process(p, f32(px), f32(py), 2, 4, None, 0, None, 0, W, W, W, C.byref(got)) == 0, L.pv_pitch_last_error(p)
    group("pitch", L.pv_pitch_last_error, p, pitch_state, [
        ("negative_channels", lambda: L.pv_pitch_process(p, f32(px), f32(py), -1, 2, None, 0, None, 0, W, W, W, None)),
        ("too_many_channels", lambda: L.pv_pitch_process(p, f32(px), f32(py), 3, 2, None, 0, None, 0, W, W, W, None)),
        ("short_hop_stride", lambda: L.pv_pitch_process(p, f32(px), f32(py), 2, 2, i32(hops["rows"]), 1, None, 0, W, W, W, None)),
        ("hop_above_fft_size", lambda: L.pv_pitch_process(p, f32(px), f32(py), 2, 2, i32(hops["above"]), 0, None, 0, W, W, W, None)),
        ("hop_0", lambda: L.pv_pitch_process(p, f32(px), f32(py), 2, 2, i32(np.array([64, 0], np.int32)), 0, None, 0, W, W, W, None)),
        ("out_capacity_too_small", lambda: L.pv_pitch_process(p, f32(px), f32(py), 2, 2, None, 0, None, 0, W, W, 10, None)),
        ("null_in", lambda: L.pv_pitch_process(p, None, f32(py), 2, 2, None, 0, None, 0, W, W, W, None)),
        ("null_out", lambda: L.pv_pitch_process(p, f32(px), None, 2, 2, None, 0, None, 0, W, W, W, None)),
        ("short_in_stride", lambda: L.pv_pitch_process(p, f32(px), f32(py), 2, 2, None, 0, None, 0, 10, W, W, None)),
        ("short_out_stride", lambda: L.pv_pitch_process(p, f32(px), f32(py), 2, 2, None, 0, None, 0, W, 10, W, None)),
        ("stretch_rejects_the_hops", lambda: L.pv_pitch_process(p, f32(px), f32(py), 2, 2, i32(hops["below"]), 0, None, 0, W, W, W, None)),
        ("stretch_rejects_the_flags", lambda: L.pv_pitch_process(p, f32(px), f32(py), 2, 2, None, 0, u8(flags["two"]), 0, W, W, W, None)),
        ("device_too_many_channels", lambda: L.pv_pitch_process_device(p, dpx, dpy, 3, 2, None, 0, None, 0, W, W, W, None)),
        ("device_out_capacity_too_small", lambda: L.pv_pitch_process_device(p, dpx, dpy, 2, 2, None, 0, None, 0, W, W, 10, None)),
        ("device_short_out_stride", lambda: L.pv_pitch_process_device(p, dpx, dpy, 2, 2, None, 0, None, 0, W, 10, W, None)),
        ("device_null_out", lambda: L.pv_pitch_process_device(p, dpx, None, 2, 2, None, 0, None, 0, W, W, W, None)),
        ("device_stretch_rejects_the_hops", lambda: L.pv_pitch_process_device(p, dpx, dpy, 2, 2, i32(hops["below"]), 0, None, 0, W, W, W, None)),
    ])
    assert L.pv_pitch_destroy(p) == 0

    # ---- every entry point on NULL and on a destroyed handle: each returns on the handle check alone.  A destroyed handle is memory that
    # free() has taken back: the library zeroes the magic word before it frees, and the calls below only READ that word, on the host (the ABI
    # has PV_ERR_DESTROYED for exactly this use).  They follow the destroy directly, before the library allocates a handle again, so that what
    # they read does not depend on the allocator handing the block out anew.
    configs = {"pv": capi.make_config(1024, 256, 1, 1), "pv_stretch": capi.make_stretch_config(256, 64, 64), "pv_resample": capi.make_resample_config(3, 2),
               "pv_pitch": capi.make_pitch_config(256, 64, 96)}
    for typ, names in DEAD_CALLS.items():
        destroy, last_error = getattr(L, typ + "_destroy"), getattr(L, typ + "_last_error")
        failed = getattr(L, typ + "_create")(None, None)                     # leaves a known text in the create buffer
        res["dead"][f"{typ}/create_null"] = failed
        dead = create(typ, configs[typ])
        res["dead"][f"{typ}_destroy/live"] = destroy(dead)
        for what, handle in (("destroyed", dead), ("null", None)):
            res["dead"][f"{typ}_destroy/{what}"] = destroy(handle)
            res["dead"][f"{typ}_last_error/{what}"] = last_error(handle).decode()
            for name in names:
                fn = getattr(L, name)
                res["dead"][f"{name}/{what}"] = fn(handle, *_null_args(fn))

    # ---- one handle per kernel family: what pv_get_info names, and how a batch is cut into chains
    def info_of(handle):
        i = capi._Info()
        assert L.pv_get_info(handle, C.byref(i)) == 0
        return i
    zeros, ones = np.zeros((3, 200 * 512), np.float32), np.ones(200, np.float32)
    for name, N, hop, flg in FAMILY_CASES:
        fh = create("pv", capi.make_config(N, hop, 3, 200, flags=flg))
        i = info_of(fh)
        rec = {"kernel_name": i.kernel_name.decode(), "threads_per_workgroup": i.threads_per_workgroup, "lds_bytes_per_workgroup": i.lds_bytes_per_workgroup,
               "compute_units": i.compute_units, "frames_per_chunk": {}}
        for nch, nhops in BATCHES:
            out = np.ones((nch, nhops * hop), np.float32)
            rc = L.pv_process_batch(fh, f32(zeros), f32(out), nch, nhops, nhops * hop, f32(ones), 0, 1)
            rec["frames_per_chunk"][f"{nch}x{nhops}"] = [rc, info_of(fh).frames_per_chunk]
            assert rc != 0 or not out.any()
        res["families"][name] = rec
        assert L.pv_destroy(fh) == 0
    for name, N, hop in RESIDENT_CASES:
        fh = create("pv", capi.make_config(N, hop, 2, 1, flags=FLAG_PERSISTENT))
        zin, zout = np.zeros((2, hop), np.float32), np.ones((2, hop), np.float32)
        zi, zo = (fp * 2)(f32(zin[0]), f32(zin[1])), (fp * 2)(f32(zout[0]), f32(zout[1]))
        quanta = []
        for _ in range(4):
            rc = L.pv_process(fh, zi, zo, 2, hop, 1.0)
            quanta.append([rc, info_of(fh).frames_per_chunk])
        assert not zout.any()
        res["resident"][name] = {"kernel_name": info_of(fh).kernel_name.decode(), "quanta": quanta}
        assert L.pv_destroy(fh) == 0
    return res


# ---------------------------------------------------------------- the tests

def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cpu_observed():
    return _on_fresh_thread(run_cpu)


@pytest.fixture(scope="module")
def gpu_observed():
    return _on_fresh_thread(run_gpu)


@pytest.mark.parametrize("name", CPU_NAMES)
def test_create_rejection(cpu_observed, name):
    want, got = _golden()["cpu"][name], cpu_observed[name]
    assert got["status"] != 0
    assert got["others_unchanged"], "a failed create wrote another handle type's create-error buffer"
    assert {k: got[k] for k in ("status", "errors")} == want


def test_create_cases_are_the_recorded_ones(cpu_observed):
    assert sorted(cpu_observed) == sorted(_golden()["cpu"])


GPU_GROUPS = ["pv_process", "pv_batch", "pv_batch_device", "pv_state", "pv_pending", "stretch_process", "stretch_link", "stretch_tempo", "stretch_onset",
              "stretch_linked", "resample", "pitch"]


@pytest.mark.gpu
@pytest.mark.parametrize("group", GPU_GROUPS)
def test_rejected_calls(gpu_observed, group):
    """Status and message of every rejected call of the group, and the state behind it bit-equal to the state before."""
    def of(d):
        return {k: v for k, v in d.items() if k.split("/")[0] == group}
    want, got = of(_golden()["gpu"]["errors"]), of(gpu_observed["errors"])
    assert want and got == want
    assert gpu_observed["unchanged"][group]


@pytest.mark.gpu
def test_rejected_calls_are_the_recorded_ones(gpu_observed):
    assert sorted(gpu_observed["errors"]) == sorted(_golden()["gpu"]["errors"])
    assert sorted(gpu_observed["unchanged"]) == sorted(GPU_GROUPS)


@pytest.mark.gpu
@pytest.mark.parametrize("typ", TYPES)
def test_dead_handles(gpu_observed, typ):
    """NULL and destroyed handles.  The per-type differences are ABI: pv_destroy(NULL) is PV_OK and a dead pv_handle gives PV_ERR_DESTROYED;
    the other three destroys give PV_ERR_ARGUMENT for NULL and PV_ERR_DESTROYED for a destroyed handle, their other entry points PV_ERR_ARGUMENT."""
    def of(d):
        return {k: v for k, v in d.items() if k.split("/")[0] in DEAD_CALLS[typ] + [typ, typ + "_destroy", typ + "_last_error"]}
    want, got = of(_golden()["gpu"]["dead"]), of(gpu_observed["dead"])
    assert len(want) == 2 * len(DEAD_CALLS[typ]) + 6 and got == want
    from phaze_amd.capi import PV_ERR_ARGUMENT, PV_ERR_DESTROYED, PV_OK
    assert got[f"{typ}_destroy/null"] == (PV_OK if typ == "pv" else PV_ERR_ARGUMENT) and got[f"{typ}_destroy/destroyed"] == PV_ERR_DESTROYED
    for name in DEAD_CALLS[typ]:
        if name not in ("pv_pitch_stretch", "pv_pitch_resampler"):
            assert got[f"{name}/null"] == got[f"{name}/destroyed"] == (PV_ERR_DESTROYED if typ == "pv" else PV_ERR_ARGUMENT), name


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c[0] for c in FAMILY_CASES])
def test_kernel_family(gpu_observed, case):
    got = gpu_observed["families"][case]
    assert all(rc == 0 for rc, _ in got["frames_per_chunk"].values())
    assert got == _golden()["gpu"]["families"][case]


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c[0] for c in RESIDENT_CASES])
def test_resident_stream(gpu_observed, case):
    got = gpu_observed["resident"][case]
    assert got["quanta"] == [[0, 1]] * 4
    assert got == _golden()["gpu"]["resident"][case]


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: PHAZE_LIB=<library to pin> python tests/test_host_contract.py --record PATH")
    import phaze_amd
    assert phaze_amd.library_path() == os.environ.get("PHAZE_LIB"), phaze_amd.library_path()
    rec = {}
    if os.path.exists(sys.argv[2]):
        with open(sys.argv[2]) as f:
            rec = json.load(f)
    rec["cpu"] = {k: {"status": v["status"], "errors": v["errors"]} for k, v in _on_fresh_thread(run_cpu).items()}
    n = C.c_int32()
    _lib().pv_device_count(C.byref(n))
    if n.value > 0:
        rec["gpu"] = _on_fresh_thread(run_gpu)
        assert all(rec["gpu"].pop("unchanged").values())
    with open(sys.argv[2], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec['cpu'])} create cases" + (f", {len(rec['gpu']['errors'])} rejected calls" if n.value > 0 else "") + f" to {sys.argv[2]}")
