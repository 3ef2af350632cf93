"""
The fastim chain's case tables (pfb_clean_amd/utils/stokes2im.py, pfb_imw_residual_weigh of csrc/imweight.hip); shared
by tests/golden/make_golden_fastim.py, test_cpu_fastim_cases.py and test_gpu_fastim.py.

KERNEL_N   the element counts of the kernel test, one per launch edge of k_residual_weigh as built.  The kernel takes
           one element per lane and trip (no vector path: a lane's complex load is 8 or 16 bytes already), BLOCK lanes per
           workgroup, at most MAX_GROUPS workgroups that stride over the array:
               1                      one lane
               63                     below one wave
               257                    two workgroups, the second with one lane at work
               CAP + 300              two grid-stride trips, the second for 300 lanes only (CAP = MAX_GROUPS * BLOCK)
           The constants below mirror the source; test_cpu_fastim_cases.py checks them against it.
CASES      the chunks of tests/golden/fastim.npz, seeded: the reference's single_stokes_image run on each, in 'single'
           and in 'double'.  Baselines stay at least four uv cells inside the counts grid at the highest frequency
           (|u| nu / c <= (nx / 2 - 4) u_cell): the reference's 6 x 6 counts footprint indexes out of bounds otherwise.
"""
import os
import types

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fastim.npz')
C_LIGHT = 299792458.0

# ---- the launch constants of k_residual_weigh (csrc/imweight.hip, entry.hpp, include/pfb_hip.h)
BLOCK = 256                     # ENTRY_BLOCK
WORK_DOUBLES = 6144             # PFB_IMW_WORK_DOUBLES
MAX_PROD = 4                    # PFB_IMW_MAX_PROD, IMW_RW_MAX_PROD
MAX_GROUPS = WORK_DOUBLES // MAX_PROD
CAP = MAX_GROUPS * BLOCK
KERNEL_N = (1, 63, 257, CAP + 300)
# which planes have a model, per nprod: none, some, all (model planes in another order than the products)
MODEL_MAPS = {1: ([-1], [0]), 2: ([-1, -1], [-1, 0], [1, 0]), 3: ([-1, -1, -1], [1, -1, 0], [2, 0, 1]),
              4: ([-1, -1, -1, -1], [-1, 1, -1, 0], [3, 2, 0, 1])}

TAGS = ('single', 'double')
EPS = {'single': 1e-5, 'double': 1e-7}          # single: gridder.EPS_MIN of float32
RESULT_KEYS = ('residual', 'wsum', 'rms', 'S', 'norm_data', 'norm_model')
UNIX_OFFSET = 3506716800.0


class Values:
    """An array under .values, as the model dataset has its variables."""

    def __init__(self, values):
        self.values = values


def opts(case, tag, **over):
    """The attributes single_stokes_image reads, for a case in a precision."""
    o = dict(precision=tag, product=case['product'], robustness=case['robustness'], filter_extreme_counts=False,
             filter_nbox=16, filter_level=10.0, nvthreads=case['nvthreads'], epsilon=EPS[tag],
             do_wgridding=case['do_wgridding'], double_accum=tag == 'double', l2reweight_dof=None, target=None)
    o.update(over)
    return types.SimpleNamespace(**o)


def even_bins(nrow, ntime):
    counts = np.array([nrow // ntime + (1 if t < nrow % ntime else 0) for t in range(ntime)], np.int64)
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64), counts


def _cnormal(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def make_model(rng, nx, ny, cell, ref_time, ref_freq, ncomps=9):
    """A component model in the form fit_image_cube's 'poly' fit returns it: value = t0 + t1 t + f1 f at t = time /
    ref_time, f = freq / ref_freq, on its own grid (here the image's)."""
    pix = rng.choice(nx * ny, ncomps, replace=False)
    coeffs = np.stack([rng.uniform(0.5, 2.0, ncomps), rng.uniform(-0.2, 0.2, ncomps), rng.uniform(-0.5, 0.5, ncomps)])
    return types.SimpleNamespace(
        coefficients=Values(coeffs), location_x=Values((pix // ny).astype(np.int64)),
        location_y=Values((pix % ny).astype(np.int64)), parametrisation='f*f1 + t*t1 + t0',
        params=Values(np.array(['t0', 't1', 'f1'])), texpr=f't/{ref_time!r}', fexpr=f'f/{ref_freq!r}', npix_x=nx,
        npix_y=ny, cell_rad_x=cell, cell_rad_y=cell, center_x=0.0, center_y=0.0)


def make_case(name, seed, nx, ny, cell, nrow, nchan, ncorr, poltype, product, *, ntime=1, wform='spectrum', jones=False,
              data2=False, flags=False, robustness=None, model=False, do_wgridding=True, nvthreads=1, nant=7):
    rng = np.random.default_rng(seed)
    freq = 1.0e9 + 2.0e7 * np.arange(nchan)
    lam = C_LIGHT / freq.max()
    u_cell, v_cell = 1 / (nx * cell), 1 / (ny * cell)
    uvw = np.stack([rng.uniform(-(nx / 2 - 4), nx / 2 - 4, nrow) * u_cell * lam,
                    rng.uniform(-(ny / 2 - 4), ny / 2 - 4, nrow) * v_cell * lam,
                    rng.uniform(-20.0, 20.0, nrow) * lam], axis=1)
    ant1 = rng.integers(0, nant - 1, nrow)
    ant2 = np.array([rng.integers(a + 1, nant) for a in ant1])
    tbin_idx, tbin_counts = even_bins(nrow, ntime)
    c = dict(name=name, nx=nx, ny=ny, cell=cell, nrow=nrow, nchan=nchan, ncorr=ncorr, poltype=poltype, product=product,
             robustness=robustness, do_wgridding=do_wgridding, nvthreads=nvthreads, freq=freq, uvw=uvw,
             utime=4.9e9 + 8.0 * np.arange(ntime), tbin_idx=tbin_idx, tbin_counts=tbin_counts,
             fbin_idx=np.array([0], np.int64), fbin_counts=np.array([nchan], np.int64),
             data=_cnormal(rng, (nrow, nchan, ncorr)).astype(np.complex64), data2=None, operator=None, sigma=None,
             weight=None, flag=None, frow=None, jones=None, mds=None, antpos=np.zeros((nant, 3)),
             radec=np.array([0.3, -0.5]))
    if wform == 'spectrum':
        c['weight'] = rng.uniform(0.5, 2.0, (nrow, nchan, ncorr)).astype(np.float32)
    elif wform == 'row':
        c['weight'] = rng.uniform(0.5, 2.0, (nrow, ncorr)).astype(np.float32)
    elif wform == 'sigma':
        c['sigma'] = rng.uniform(0.5, 2.0, (nrow, nchan, ncorr)).astype(np.float32)
    if data2:
        c['data2'], c['operator'] = (0.5 * _cnormal(rng, (nrow, nchan, ncorr))).astype(np.complex64), '-'
    if flags:
        ant2[::9] = ant1[::9]                                    # autocorrelations
        c['flag'] = rng.uniform(size=(nrow, nchan, ncorr)) < 0.05
        c['frow'] = rng.uniform(size=nrow) < 0.1
    if jones:                                                    # QuartiCal's layout, the diagonal
        amp = rng.uniform(0.5, 2.0, (ntime, nchan, nant, 1, 2))
        c['jones'] = (amp * np.exp(2j * np.pi * rng.uniform(size=amp.shape))).astype(np.complex64)
    if model:
        c['fbin_idx'], c['fbin_counts'] = np.array([0, 2], np.int64), np.array([2, 1], np.int64)
        c['mds'] = make_model(rng, nx, ny, cell, float(c['utime'][0]), float(freq[0]))
    c['ant1'], c['ant2'] = ant1.astype(np.int32), ant2.astype(np.int32)
    return c


def _build():
    return [
        make_case('linear-I', 11, 32, 24, 0.012, 63, 3, 4, 'linear', 'I'),
        make_case('jones-sigma-minus', 12, 16, 64, 0.008, 260, 4, 4, 'linear', 'Q', ntime=2, wform='sigma', jones=True,
                  data2=True, flags=True, robustness=0.0, nvthreads=2),
        make_case('model-two-bins', 13, 32, 24, 0.012, 131, 3, 4, 'linear', 'I', robustness=-1.0, model=True),
        make_case('circular-V-nowgrid', 14, 16, 64, 0.008, 97, 5, 2, 'circular', 'V', wform='none',
                  do_wgridding=False),
        make_case('row-weights', 15, 32, 24, 0.012, 150, 3, 4, 'linear', 'U', wform='row', robustness=1.0),
    ]


CASES = _build()
CASE_IDS = [c['name'] for c in CASES]


def case_named(name):
    return CASES[CASE_IDS.index(name)]


COLUMNS = ('data', 'data2', 'operator', 'ant1', 'ant2', 'uvw', 'frow', 'flag', 'sigma', 'weight', 'mds', 'jones', 'nx',
           'ny', 'freq', 'utime', 'tbin_idx', 'tbin_counts', 'fbin_idx', 'fbin_counts', 'radec', 'antpos', 'poltype')


def _column(a, tag):
    """A copy of the array; data, weights and Jones terms in the type of the precision.  Every such value is exactly
    representable in fp32 and drawn so: one table serves both precisions and a comparison sees arithmetic error only.
    (A float32 sigma column in a 'double' run would have the reference form 1 / sigma^2 in fp32 under the generator's
    stand-in for numexpr, which evaluates in numpy's types.)"""
    if not isinstance(a, np.ndarray):
        return a
    if a.dtype == np.complex64:
        return a.astype(np.complex64 if tag == 'single' else np.complex128)
    if a.dtype == np.float32:
        return a.astype(np.float32 if tag == 'single' else np.float64)
    return a.copy()


def call_kwargs(case, tag, **over):
    """The keywords of single_stokes_image for a case in a precision (copies of the arrays: the reference writes into
    some of them)."""
    kw = {k: _column(case[k], tag) for k in COLUMNS}
    kw.update(opts=opts(case, tag), cell_rad=case['cell'], fieldid=0, ddid=1, scanid=2, bandid=3, timeid=4,
              fds_store='unused', wid=None)
    kw.update(over)
    return kw


def live_mask(case):
    """(nrow, nchan) bool: the visibilities that no flag, flagged row or autocorrelation takes out."""
    dead = case['ant1'] == case['ant2']
    if case['frow'] is not None:
        dead = dead | case['frow']
    dead = np.broadcast_to(dead[:, None], (case['nrow'], case['nchan']))
    if case['flag'] is not None:
        dead = dead | case['flag'].any(axis=2)
    return ~dead


def cube_dataset(seed=21):
    """A dataset of 3 output times x 2 bands for stokes_image_cube: six unique times of unequal row counts, two per
    output time; four channels in bins of one, two bins per image; diagonal Jones terms, weights, flags, a model."""
    c = make_case('cube', seed, 32, 24, 0.012, 121, 4, 4, 'linear', 'I', ntime=6, jones=True, flags=True, robustness=0.0,
                  model=True)
    c.update(time_mapping={'start_indices': np.array([0, 2, 4]), 'counts': np.array([2, 2, 2])},
             row_mapping={'start_indices': c['tbin_idx'], 'counts': c['tbin_counts']},
             freq_mapping={'start_indices': np.arange(4), 'counts': np.ones(4, np.int64)}, cpgi=2, cpdi=1)
    return c


_golden = None


def golden(name, tag):
    """The reference's results of a case: residual (nx, ny) float64, wsum, rms and the scalars of the bounds -- S =
    sum over the unflagged visibilities of weight (|Stokes vis| + |model vis|), norm_data = |R^H W vis|, norm_model =
    |R^H W R model| (0 without a model)."""
    global _golden
    if _golden is None:
        with np.load(GOLDEN, allow_pickle=False) as g:
            _golden = {k: g[k] for k in g.files}
    return {k: _golden[f'{name}_{tag}_{k}'] for k in RESULT_KEYS}
