"""CPU: mio_hip_llm_generate_queue (include/mio_hip.h) refuses a NULL handle with MIO_ERR_INVALID
and an error text, before it touches a device; the Python binding declares the call and its
stats struct as the header does."""
import ctypes
import os

import miotts_amd as m


def test_generate_queue_null_handle_is_invalid():
    L = m.lib()
    rc = L.mio_hip_llm_generate_queue(None, None, None, 1, 1, 1, 0.8, None, -1, -1, -1, -1, None, None, None)
    assert rc == -1
    assert b"llm_generate_queue" in L.mio_hip_last_error()


def test_queue_stats_struct_matches_the_header():
    src = open(os.path.join(m.INCLUDE_DIR, "mio_hip.h"), encoding="utf-8").read()
    assert "typedef struct mio_llm_queue_stats" in src and "mio_hip_llm_generate_queue" in src
    names = [n for n, _ in m.QueueStats._fields_]
    assert names == ["steps", "live_slot_steps", "refills", "prefill_chunks", "slot_of", "start_step"]
    body = src[src.index("typedef struct mio_llm_queue_stats"):src.index("} mio_llm_queue_stats;")]
    assert [body.index(n + ";") for n in names] == sorted(body.index(n + ";") for n in names)
    assert ctypes.sizeof(m.QueueStats) == 4 * 4 + 2 * ctypes.sizeof(ctypes.c_void_p)
