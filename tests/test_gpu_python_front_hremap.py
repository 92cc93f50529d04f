"""The Python front of mifc_hremap_* on the GPU (mi-fieldcalc_amd/hremap.py): the same call with host arrays and with device
tensors -- the table and the fields -- gives equal bits and equal flags, and both equal the restatement."""
import numpy as np
import pytest

import hremap_restate as hr
from cases import same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode,min_frac", [("strict", 0.0), ("renorm", 0.5)])
def test_host_arrays_against_device_tensors(gpu_ctx, mode, min_frac):
    import torch

    from mi_fieldcalc_amd import hremap

    fields, (rowptr, col, w) = hr.main_case(nf=3, nlev=5, ny=12, nx=16, ndst=330, seed=17)
    flags = np.random.default_rng(17).choice([hr.ALL_DEFINED, hr.SOME_DEFINED, hr.NONE_DEFINED], size=(3, 5)).astype(np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    exp, efd = hr.remap(fields, rowptr, col, w, mode, min_frac, flags)
    with hremap.Plan(gpu_ctx, rowptr, col, w, nsrc=192) as hplan, hremap.Plan(gpu_ctx, dev(rowptr), dev(col), dev(w), nsrc=192) as dplan:
        assert hplan.info() == dplan.info() and hplan.ndst == dplan.ndst == 330
        results = []
        for plan in (hplan, dplan):
            h, hfd = hremap.hremap_levels(gpu_ctx, plan, fields, mode, min_frac, fdefined_in=flags, dst_shape=(10, 33))
            d, dfd = hremap.hremap_levels(gpu_ctx, plan, dev(fields), mode, min_frac, fdefined_in=flags, dst_shape=(10, 33))
            assert isinstance(h, np.ndarray) and d.is_cuda and h.shape == tuple(d.shape) == (3, 5, 10, 33)
            results += [(h, hfd), (d.cpu().numpy(), dfd)]
        for got, fd in results:
            assert same_bits(got.reshape(exp.shape), exp, nan_payload=False) and np.array_equal(fd, efd)
        # one batch, listed batches and ESMF triples give the same bits too
        one, ofd = hremap.hremap_levels(gpu_ctx, dplan, dev(fields[1]), mode, min_frac, fdefined_in=flags[1])
        assert tuple(one.shape) == (5, 330) and ofd.shape == (5,)
        assert same_bits(one.cpu().numpy(), exp[1], nan_payload=False) and np.array_equal(ofd, efd[1])
        form = hremap.last_hremap_form(gpu_ctx)
        assert form["mode"] == mode and form["width"] == hplan.info()["max_row"]
    rows = np.repeat(np.arange(330), np.diff(rowptr))
    keep = np.lexsort((np.arange(rows.size), rows % 7))  # the rows out of order, the entries of a row in their order
    assert (np.diff(rows[keep]) < 0).any()
    with hremap.Plan.from_coo(gpu_ctx, rows[keep] + 1, col[keep] + 1, w[keep], 192, 330, one_based=True) as plan:
        got, fd = hremap.hremap_levels(gpu_ctx, plan, fields, mode, min_frac, fdefined_in=flags)
        assert same_bits(got, exp, nan_payload=False) and np.array_equal(fd, efd)
