"""CPU: host-side logic of the static-shape plan (capacities, overflow check) -- no kernels involved."""
import pytest
import torch


def test_static_plan_capacities_and_overflow():
    from com_amd import ops, _lib
    plan = ops.StaticPlan(margin=1.25, round_to=1024)
    with pytest.raises(_lib.PcdError):
        plan.cap("voxels")                                  # nothing observed yet
    plan.observe("voxels", 340000)
    plan.observe("voxels", 337000)                          # keeps the maximum
    plan.observe(("conv", "spconv2"), 297001)
    assert plan.caps["voxels"] == 340000
    cap = plan.cap("voxels")
    assert cap % 1024 == 0 and 425000 <= cap <= 427000      # 1.25 x, rounded up to 1024
    assert plan.cap(("conv", "spconv2")) >= 1.25 * 297001
    # overflow detection reads the device-side counts recorded during the captured step
    plan.record("voxels", torch.tensor([339000], dtype=torch.int32), cap)
    assert plan.check()
    plan.record(("conv", "spconv2"), torch.tensor([5, 999999], dtype=torch.int32), 400000)   # last entry = total
    with pytest.raises(_lib.PcdError):
        plan.check()


def test_rulebook_inverse_and_helpers_are_host_safe():
    from com_amd import ops
    assert ops.pow2_ge8(5) == 8 and ops.pow2_ge8(16) == 16 and ops.pow2_ge8(65) == 128
    assert ops._triple(3) == [3, 3, 3] and ops._triple((3, 1, 1)) == [3, 1, 1]


def test_rulebook_built_by_keyword_declares_all_of_its_state():
    """Every attribute the convs, the backward passes and the prefetcher read exists from __init__ on, with its documented
    default; the lazy tables of an empty rulebook stay None (no kernel to run); construction is by keyword only."""
    from com_amd import ops
    geo = dict(ksize=[3, 3, 3], stride=[2, 2, 2], padding=[1, 1, 1], dilation=[1, 1, 1])
    rb = ops.Rulebook(subm=False, kvol=27, n_in=0, n_out=0, **geo)
    defaults = dict(n_in_dev=None, n_out_dev=None, nbr_out_packed=None, nbr_cls=None, out_indices=None, out_shape=None,
                    rank=None, order=None, classes=None, implicit_pairs=False, ready_event=None, joined_stream=None,
                    _win_plans={}, _nbr_out=None, _nbr_in=None, _pairs=None, _pair_num=None, _finish_tables=None)
    for name, value in defaults.items():
        assert name in vars(rb) and vars(rb)[name] == value, name
    assert set(vars(rb)) == set(defaults) | {"subm", "kvol", "n_in", "n_out"} | set(geo)
    assert rb.nbr_out is None and rb.nbr_buffer is None and rb.nbr_in is None and rb.pairs is None and rb.pair_num is None
    assert rb.nbr_complete
    a, b = ops.Rulebook(subm=True, kvol=27, n_in=0, n_out=0, **geo), ops.Rulebook(subm=True, kvol=27, n_in=0, n_out=0, **geo)
    a._win_plans[(32, 16)] = "plan"
    assert b._win_plans == {}                                  # (one cache per rulebook)
    with pytest.raises(TypeError):
        ops.Rulebook(False, 27, 0, 0, None, None, None, None, None, None, *geo.values())
    # the same values reach the object whatever their keyword order; inverse() swaps the two sides
    t = [torch.zeros(1, dtype=torch.int32) for _ in range(4)]
    rb = ops.Rulebook(order=ops.ROWS_YXZ, n_out_dev=t[3], n_in_dev=t[2], nbr_in=t[1], nbr_out=t[0],
                      out_shape=(5, 6, 7), subm=False, kvol=27, n_in=3, n_out=2, **geo)
    assert rb.nbr_out is t[0] and rb.nbr_in is t[1] and rb.out_shape == [5, 6, 7] and rb.order == ops.ROWS_YXZ
    inv = rb.inverse()
    assert (inv.n_in, inv.n_out, inv.kvol, inv.subm) == (2, 3, 27, False) and inv.nbr_out is t[1] and inv.nbr_in is t[0]
    assert inv.n_in_dev is t[3] and inv.n_out_dev is t[2] and inv.pairs is None and inv.order is None and inv.rank is None
    assert (inv.ksize, inv.stride, inv.padding, inv.dilation) == (rb.ksize, rb.stride, rb.padding, rb.dilation)
    red = ops.BnReduce(1)
    assert (red.partial, red.rows, red.partial_rows, red.partial_keep) == (None, 0, 0, None)


@pytest.mark.parametrize("extra", [(4,), (0, 1, 24), (4, 0, 0, 5)], ids=["7", "9", "10"])
def test_wgrad_job_record_fills_the_c_struct_like_the_old_tuples(extra):
    """ops.WgradJob -> PcdWgradReduceJob: field for field what wgrad_reduce_batched decoded from the tuples of 7 / 9 / 10
    elements the producers used to append (missing trailing elements = 0); such a plain tuple is still accepted."""
    from com_amd import ops, _lib
    ws, dw = torch.zeros(8, dtype=torch.uint8), torch.zeros(8)
    old = (ws, dw, 27, 16, 32, 1000) + extra
    expect = [ws.data_ptr(), dw.data_ptr()] + list(old[2:]) + [0] * (10 - len(old))
    names = [f for f, _ in _lib.PcdWgradReduceJob._fields_]
    assert names == list(ops.WgradJob._fields)
    job = ops.WgradJob(ws, dw, kvol=27, cin=16, cout=32, pmax=1000,
                       **dict(zip(("splits", "layout", "cout_write", "cin_write"), extra)))
    for made in (ops._wgrad_job_struct(job), ops._wgrad_job_struct(old)):
        assert [getattr(made, f) for f in names] == expect
    with pytest.raises(TypeError):
        ops._wgrad_job_struct(old[:5])                         # (not a job: too short)
