"""Which chain and output-stage kernels a block gets (choose_chain / choose_post behind ow_test_block_plan): the table of pool sizes,
builds and switches, pinned on the host -- no device, no pool.  The expectations are the conditions of the launch ladders the two
functions replaced, written down by hand."""
import ctypes as C

import pytest

LEGACY, MELANGE = 0, 1            # preamp kind (OW_PREAMP_LEGACY8 / OW_PREAMP_MELANGE12)
BEHAVIORAL, MELANGE_PA = 0, 1     # power amp kind (OW_POWER_AMP_BEHAVIORAL / OW_POWER_AMP_MELANGE)


def plan(L, ne, *, preamp=LEGACY, amp=BEHAVIORAL, os=True, sparse=True, block=512, pinned=False, sw=None, cap=128):
    out = C.create_string_buffer(cap)
    rc = L.ow_test_block_plan(preamp, amp, int(os), int(sparse), ne, block, int(pinned), sw.encode() if sw is not None else None, out, cap)
    return out.value.decode() if rc == 0 else rc


def post_by_size(ne, os=True):
    if not os:
        return "k_post<false>"
    return "k_post<false,true>" if ne >= 131072 else "k_post<true>"


@pytest.mark.parametrize("os", [True, False])
def test_legacy_ladder_by_pool_size(hiplib_host, os):
    t = "true" if os else "false"
    for ne in (1, 64, 1024):
        assert plan(hiplib_host, ne, os=os, block=128) == f"k_chain_row<{t},8>"
        assert plan(hiplib_host, ne, os=os, block=129) == f"k_chain_row<{t},16>"
        assert plan(hiplib_host, ne, os=os, block=64) == f"k_chain_row<{t},8>"
        assert plan(hiplib_host, ne, os=os, block=512) == f"k_chain_row<{t},16>"
    for ne in (1025, 2048):
        for block in (128, 129):
            assert plan(hiplib_host, ne, os=os, block=block) == f"k_chain_fused<{t}>"
    for ne in (2049, 4096):
        assert plan(hiplib_host, ne, os=os) == f"k_preamp_wide + k_post<{t}>"
    for ne in (4097, 8192, 131071):
        assert plan(hiplib_host, ne, os=os) == f"k_preamp + k_post<{t}>"
    for ne in (131072, 200000):
        assert plan(hiplib_host, ne, os=os) == "k_preamp_pair + " + ("k_post<false,true>" if os else "k_post<false>")


def test_block_to_a_pinned_host_block_streams_above_the_quad_sizes(hiplib_host):
    for ne in (4097, 8192, 131071, 131072):                # the stream kernel wins over the pair
        assert plan(hiplib_host, ne, pinned=True) == "k_chain_stream"
    assert plan(hiplib_host, 1024, pinned=True, block=128) == "k_chain_row<true,8>"
    assert plan(hiplib_host, 1025, pinned=True) == "k_chain_fused<true>"
    assert plan(hiplib_host, 2049, pinned=True) == "k_preamp_wide + k_post<true>"
    assert plan(hiplib_host, 4096, pinned=True) == "k_preamp_wide + k_post<true>"


def test_no_stream_kernel_without_oversampling(hiplib_host):
    for ne in (4097, 8192, 131072):
        for sw in (None, "chain_stream=1"):
            for pinned in (False, True):
                got = plan(hiplib_host, ne, os=False, pinned=pinned, sw=sw)
                assert got == ("k_preamp_pair" if ne >= 131072 else "k_preamp") + " + k_post<false>"
    assert plan(hiplib_host, 64, os=False, sw="chain_fused=0,preamp_wide=0,chain_stream=1") == "k_preamp + k_post<false>"


@pytest.mark.parametrize("ne", [1, 64, 1024, 2048, 4096, 4097, 131071, 131072])
def test_melange_preamp_is_never_fused_or_streamed(hiplib_host, ne):
    L = hiplib_host
    post = post_by_size(ne)
    for extra in ("", "chain_fused=1", "chain_stream=1", "chain_fused=1,chain_row=1", "preamp_wide=1", "preamp_pair=1"):
        def p(sw="", **kw):
            both = ",".join(x for x in (extra, sw) if x)
            return plan(L, ne, preamp=MELANGE, sw=both or None, **kw)
        for pinned in (False, True):
            assert p(pinned=pinned) == f"k_preamp_mel_col + {post}"
            assert p(pinned=pinned, sparse=False) == f"k_preamp_mel_lit + {post}"
        assert p("mel_eng=1") == f"k_preamp_mel_eng + {post}"
        assert p("mel_eng=1", sparse=False) == f"k_preamp_mel_lit + {post}"
        assert p("mel_eng=1,mel_lds=1") == f"k_preamp_mel_lit + {post}"
        assert p("mel_lds=1") == f"k_preamp_mel_lit + {post}"
        assert p("mel_generic=1") == f"k_preamp_mel_col + {post}"
        for others in ("", ",mel_eng=1", ",mel_lds=1", ",mel_eng=1,mel_lds=1"):
            assert p("mel_rank1=1" + others) == f"k_preamp_mel + {post}"
            assert p("mel_rank1=1" + others, sparse=False) == f"k_preamp_mel + {post}"
    assert plan(L, ne, preamp=MELANGE, os=False) == "k_preamp_mel_col + k_post<false>"
    assert plan(L, ne, preamp=MELANGE, amp=MELANGE_PA) == "k_preamp_mel_col + k_post_mpa"


def test_melange_power_amp_is_never_fused_or_streamed(hiplib_host):
    L = hiplib_host
    for sw in (None, "chain_fused=1", "chain_stream=1", "chain_fused=1,chain_row=1", "post_pair=1"):
        for pinned in (False, True):
            for os in (True, False):
                for ne in (1, 1024, 2048, 4096):
                    assert plan(L, ne, amp=MELANGE_PA, os=os, pinned=pinned, sw=sw) == "k_preamp_wide + k_post_mpa"
                for ne in (4097, 131071):
                    assert plan(L, ne, amp=MELANGE_PA, os=os, pinned=pinned, sw=sw) == "k_preamp + k_post_mpa"
                assert plan(L, 131072, amp=MELANGE_PA, os=os, pinned=pinned, sw=sw) == "k_preamp_pair + k_post_mpa"


def test_forced_switches(hiplib_host):
    L = hiplib_host
    assert plan(L, 5000, sw="chain_fused=1") == "k_chain_fused<true>"
    assert plan(L, 5000, os=False, sw="chain_fused=1") == "k_chain_fused<false>"
    assert plan(L, 5000, sw="chain_fused=1,chain_row=1", block=128) == "k_chain_row<true,8>"
    assert plan(L, 5000, sw="chain_fused=1,chain_row=1", block=129) == "k_chain_row<true,16>"
    assert plan(L, 5000, sw="chain_row=1") == "k_preamp + k_post<true>"            # the row only inside the fused launch
    assert plan(L, 64, sw="chain_row=0") == "k_chain_fused<true>"
    assert plan(L, 64, sw="chain_fused=0") == "k_preamp_wide + k_post<true>"
    assert plan(L, 64, sw="chain_fused=0,preamp_wide=0,chain_stream=1") == "k_chain_stream"
    assert plan(L, 64, sw="chain_fused=0,preamp_wide=0") == "k_preamp + k_post<true>"
    assert plan(L, 64, pinned=True, sw="chain_fused=0,preamp_wide=0") == "k_chain_stream"
    assert plan(L, 8192, pinned=True, sw="chain_stream=0") == "k_preamp + k_post<true>"
    assert plan(L, 64, sw="chain_fused=0,preamp_wide=0,preamp_pair=1,post_pair=1") == "k_preamp_pair + k_post<false,true>"
    assert plan(L, 64, sw="chain_fused=0,preamp_wide=0,preamp_pair=1") == "k_preamp_pair + k_post<true>"
    assert plan(L, 64, sw="chain_fused=0,preamp_wide=0,post_pair=1") == "k_preamp + k_post<false,true>"
    assert plan(L, 64, os=False, sw="chain_fused=0,preamp_wide=0,post_pair=1") == "k_preamp + k_post<false>"
    assert plan(L, 200000, os=False, sw="post_pair=1") == "k_preamp_pair + k_post<false>"
    assert plan(L, 200000, sw="preamp_pair=0,post_pair=0") == "k_preamp + k_post<true>"
    assert plan(L, 8192, sw="preamp_wide=1") == "k_preamp_wide + k_post<true>"
    assert plan(L, 1024, sw="preamp_wide=0") == "k_preamp + k_post<true>"          # by size the fused launch follows the quad preamp
    assert plan(L, 64, sw="chain_fused=-1,chain_row=-1", block=128) == "k_chain_row<true,8>"    # negative: back to the size rule


def test_error_cases(hiplib_host):
    L = hiplib_host
    assert plan(L, 64, sw="no_such_switch=1") == -1
    assert plan(L, 64, sw="chain_row=0,no_such_switch=1") == -1
    assert plan(L, 64, sw="chain_row") == -1
    assert plan(L, 64, sw="pa_sort=3") == -1                 # a value the switch refuses
    assert plan(L, 64, sw="pa_sort=2") == "k_chain_row<true,16>"
    full = "k_preamp_pair + k_post<false,true>"
    assert plan(L, 131072, cap=len(full) + 1) == full
    assert plan(L, 131072, cap=len(full)) == -1              # no room for the terminator
    assert plan(L, 131072, cap=1) == -1
