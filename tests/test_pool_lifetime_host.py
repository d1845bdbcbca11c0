"""The two resource hooks of openwurli_hip_test.h on the host side: they bind, and a pool that cannot be created leaves nothing behind."""
import ctypes as C


def test_resource_hooks_bind_and_a_refused_create_owns_nothing(hiplib_host):
    from openwurli_amd import binding
    L = hiplib_host
    before = L.ow_test_live_resources()
    L.ow_test_fail_acquire_after(3)
    L.ow_test_fail_acquire_after(-1)                       # armed and disarmed again: nothing below is injected
    L.ow_clear_error()
    h = L.ow_pool_new_kinds(48000.0, 1, 0, 0, 0, 1)        # legacy LFO tremolo: no process-wide trajectory store behind the pool
    if h:                                                  # a machine with a device: the pool exists, and gives everything back
        assert L.ow_test_live_resources() > before
        L.ow_pool_free(C.c_void_p(h))
        assert L.ow_test_live_resources() == before
    else:
        err = binding.take_error(L)       # the library's own refusal, or the runtime's when not even the device count can be had
        assert "no HIP device" in err or "no ROCm-capable device" in err, err
        assert L.ow_test_live_resources() == before == 0
    assert L.ow_pool_new(0.0, 1, 0, 0) is None and "invalid sample rate" in binding.take_error(L)
    assert L.ow_test_live_resources() == before
