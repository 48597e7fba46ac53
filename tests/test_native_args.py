"""Host-side argument checks of the native wrappers (CPU: they raise before any device work), and
of the native layers beneath them.

The native layers take their arguments by name through one reader (csrc/pyargs.h): a missing
key, a key nothing reads and a value of the wrong Python type are a TypeError that names the entry
point and the key, raised before anything runs. Through ``_host`` (always buildable) and, where the
extension is built, through ``_C`` -- there only along paths that raise before any launch, so no
device is needed and no entry point is called with a complete argument set."""
import pytest
import torch

from macbf_gnn_amd.ops import host, native


@pytest.mark.parametrize("lanes", [1, 2, 5, 16])
def test_scan_rejects_unsupported_lane_layouts(lanes):
    S = torch.zeros(1, 16, 4)
    idx = torch.zeros(1, 16, 12, dtype=torch.int32)
    with pytest.raises(native.NativeError, match="lanes"):
        native.scan(S, idx, None, None, None, K=12, lanes=lanes)


def test_edge_backward_grid_one_workgroup_per_cu_for_x3(monkeypatch):
    """The x3 edge backward holds one workgroup per CU: its grid is capped at the CU count
    (the 16-bit builds at two per CU); MACBF_EDGE_WG_PER_CU overrides."""
    monkeypatch.setattr(native, "num_cu", lambda device=None: 256)
    monkeypatch.delenv("MACBF_EDGE_WG_PER_CU", raising=False)
    monkeypatch.delenv("MACBF_NODE_CHUNK", raising=False)
    agents = 64 * 1024
    _, e_x3 = native.ctrl_bwd_grids(agents, None, "fp32")
    _, e_bf = native.ctrl_bwd_grids(agents, None, "bf16")
    assert e_x3 == 256 and e_bf == 512
    monkeypatch.setenv("MACBF_EDGE_WG_PER_CU", "2")
    assert native.ctrl_bwd_grids(agents, None, "fp32")[1] == 512


def test_scan_plans_of_the_production_configs():
    """The scan launcher's plan (csrc/scan.hip mb_scan_plan; host logic, no launch) for the
    BASELINE shapes at 256 CUs: the instantiations tests/test_gpu_scan_plans.py pins to the oracle."""
    p = native.scan_plan(64, 1024, 12, prev=True)
    assert (p["bs"], p["lpa"], p["use_cells"], p["cell_g"]) == (1024, 4, 1, 24)
    p = native.scan_plan(64, 1024, 12, Nn=1120, dim=3, prev=True)
    assert (p["bs"], p["lpa"], p["use_cells"], p["cell_g"], p["wave_atomic"]) == (512, 4, 1, 10, 1)
    p = native.scan_plan(8, 1024, 12, prev=True)
    assert (p["bs"], p["lpa"], p["use_cells"], p["cell_g"]) == (256, 8, 1, 16)
    p = native.scan_plan(1, 20000, 12, prev=True)
    assert p["glb"] == 1 and p["cells"] == 0


def test_scan_cell_lds_only_when_searched():
    """Safety-only scans (the rollout's tail) and first steps (no temporal bound) never search
    the cell grid and do not allocate its LDS."""
    base = native.scan_plan(64, 1024, 12, prev=True)
    for kw in (dict(do_knn=False, prev=True), dict(prev=False)):
        p = native.scan_plan(64, 1024, 12, **kw)
        assert p["cells"] == 0 and p["use_cells"] == 0 and p["lds"] < base["lds"], kw
    assert base["cells"] == 1 and base["lds"] <= 160 * 1024


# ----------------------------------------------------------------------------- named arguments
MPD = dict(p=0, n=0, dim=2, stride=2, L=1.0, cutoff=1.0)


def test_host_extra_key_names_key_and_function():
    with pytest.raises(TypeError, match=r"min_pair_distance: unexpected argument 'cutof'"):
        host.lib().min_pair_distance(**MPD, cutof=2.0)


def test_host_missing_key_names_key_and_function():
    kw = dict(MPD)
    del kw["stride"]
    with pytest.raises(TypeError, match=r"min_pair_distance: missing argument 'stride'"):
        host.lib().min_pair_distance(**kw)


def test_host_wrong_type_names_the_key():
    with pytest.raises(TypeError, match=r"min_pair_distance: argument 'n' must be int, got str"):
        host.lib().min_pair_distance(**dict(MPD, n="3"))
    with pytest.raises(TypeError, match=r"argument 'dim' must be int, got float"):
        host.lib().min_pair_distance(**dict(MPD, dim=2.0))
    with pytest.raises(TypeError, match=r"argument 'p' must be a non-negative int, got int"):
        host.lib().min_pair_distance(**dict(MPD, p=-1))
    with pytest.raises(TypeError):
        host.lib().min_pair_distance(0, 0, 2, 2, 1.0, 1.0)          # no positional form is left


def test_host_correct_call():
    p = torch.tensor([[0.0, 0.0], [3.0, 4.0], [0.0, 0.5]])
    assert host.min_pair_distance(p) == 0.5
    assert host.lib().min_pair_distance(p=p.data_ptr(), n=3, dim=2, stride=2, L=5.0, cutoff=1.0) == 0.5


@pytest.fixture(scope="module")
def ext():
    if not native.available():
        pytest.skip("extension not built (python csrc/build.py)")
    return native.lib()


def test_ext_extra_and_missing_keys(ext):
    csr = dict(idx=0, G=1, N=1, K=1, Nn=1, ptr=0, edges=0, ws=0)
    with pytest.raises(TypeError, match=r"rev_csr: missing argument 'stream'"):
        ext.rev_csr(**csr)
    with pytest.raises(TypeError, match=r"rev_csr: missing argument 'K'"):
        ext.rev_csr(idx=0, G=1, N=1)
    with pytest.raises(TypeError, match=r"ctrl_edge_bwd: missing argument 'S'"):
        ext.ctrl_edge_bwd(prec=0)
    with pytest.raises(TypeError, match=r"cbf_dh: argument 'lc' must be a tuple of 7 or 8, got int"):
        ext.cbf_dh(h=0, hmask=0, map1=0, src=0, nev=0, dang=0, valid=0, B=1, T=1, N=1, K=1, counts=0, lc=3)
    with pytest.raises(TypeError, match=r"pack_gather: argument 'commit' must be a dict, got tuple"):
        ext.pack_gather(src=0, n=0, idx16=0, m16=0, out16=0, f16=0, idx32=0, m32=0, out32=0, commit=(1, 2))
    with pytest.raises(TypeError, match=r"pack_gather: unexpected argument 'oK'"):
        ext.pack_gather(src=0, n=0, idx16=0, m16=0, out16=0, f16=0, idx32=0, m32=0, out32=0,
                        commit=dict(ok=0, steps=0, mask=0, ngroups=1, skipped=0, gscale=0, good=0, growth=1,
                                    max_scale=1.0, stats_row=0, oK=0))


def _zeros(keys):
    return dict.fromkeys(keys, 0)


# the drivers' own keys (csrc/runtime.cpp) and the fields of the structs their sub-dicts fill (csrc/fill.h)
ROLLOUT_OWN = ("Tmax resort_every check_every hfwd_blocks num_cu prec host_dist done_thr publish poll_query_ms small_ctl "
               "small_apw knn_tail small_stamps node_acts node_act_bytes").split()
BPTT_OWN = "Tmax prec nb_node nb_edge step_rows node_part edge_part fused_step node_acts node_act_bytes dS Gb rptr redges".split()
SORT_KEYS = "S s_env B N rec L perm".split()
SCAN_KEYS = ("S s_env perm B N K Nn dim idx i_env dang cnt c_env safe sf_env r2_train ttc_train r2_check ttc_check do_knn "
             "do_safety prev_idx pi_env ws ws_env lanes stamps").split()
CTRL_KEYS = ("S s_env dim G idx i_env B N K wpack f_edge f_node wvec A a_env Snext sn_env dist_sum d_env act_sum ac_env "
             "noise n_env noise_key noise_prob noise_scale noise_t dt obs_r sqrt3 pooled p_env argmax am_env apw stamps").split()
EDGE_KEYS = "S s_env dim idx i_env argmax am_env dP dp_env B N K wpack f_ew1f f_ew2tn dEc de_env partial init qsplit".split()


def test_ext_drivers_and_commit_dict(ext):
    # an empty commit dict is a dict with every key missing, not None
    with pytest.raises(TypeError, match=r"pack_gather: missing argument 'ok'"):
        ext.pack_gather(src=0, n=0, idx16=0, m16=0, out16=0, f16=0, idx32=0, m32=0, out32=0, commit={})
    # argument errors come before the groups are looked at (an empty list is refused without a launch)
    adam = dict(param=0, grad=0, m=0, v=0, b1=0.9, b2=0.99, eps=1e-8, wd=0.0, ok=0, lr=1e-3, stream=0)
    with pytest.raises(TypeError, match=r"adam_multi: unexpected argument 'lr_'"):
        ext.adam_multi(groups=[], lr_=1.0, **adam)
    # the fused step takes none of the single launches' 16x16x32 extras
    with pytest.raises(native.NativeError, match="ctrl_bwd_step: the fused kernel takes no 16x16x32 images"):
        native.ctrl_bwd_step(dict(wrm16=torch.zeros(1)), {}, 1)
    with pytest.raises(native.NativeError, match="no edge stamps"):
        native.ctrl_bwd_step({}, dict(stamps=torch.zeros(1)), 1)
    # the drivers read their config dicts the same way, before they touch the device
    with pytest.raises(TypeError, match=r"RolloutDriver: missing argument 'Tmax'"):
        ext.RolloutDriver({})
    with pytest.raises(TypeError, match=r"BpttDriver: argument 'Tmax' must be int, got str"):
        ext.BpttDriver({"Tmax": "2"})
    # a key nothing reads is refused, by both training drivers (a complete config of zeros gets as far as
    # the dimension check, still before any device call)
    roll = dict(_zeros(ROLLOUT_OWN), hfwd=None, cell_sort=_zeros(SORT_KEYS), scan=_zeros(SCAN_KEYS), ctrl=_zeros(CTRL_KEYS))
    bptt = dict(_zeros(BPTT_OWN), node=dict(_zeros(NODE_KEYS), act_coef=0.0, dt=0.0, sqrt3=0.0), edge=_zeros(EDGE_KEYS))
    with pytest.raises(ValueError, match="RolloutDriver: bad dimensions"):
        ext.RolloutDriver(roll)
    with pytest.raises(ValueError, match="BpttDriver: bad dimensions"):
        ext.BpttDriver(bptt)
    with pytest.raises(TypeError, match=r"RolloutDriver: unexpected argument 'check_evry'"):
        ext.RolloutDriver(dict(roll, check_evry=1))
    with pytest.raises(TypeError, match=r"BpttDriver: unexpected argument 'gscale'"):
        ext.BpttDriver(dict(bptt, gscale=0))
    # a sub-dict is read by the launcher's own fill function, under the driver's and its own name
    with pytest.raises(TypeError, match=r"RolloutDriver ctrl: missing argument 'apw'"):
        ext.RolloutDriver(dict(roll, ctrl=_zeros(k for k in CTRL_KEYS if k != "apw")))
    with pytest.raises(TypeError, match=r"RolloutDriver scan: unexpected argument 'num_cu'"):
        ext.RolloutDriver(dict(roll, scan=dict(roll["scan"], num_cu=1)))
    with pytest.raises(TypeError, match=r"BpttDriver edge: missing argument 'S'"):
        ext.BpttDriver(dict(bptt, edge={}))
    # hfwd=None (no overlapped CBF slices) is accepted: the next key is asked for
    with pytest.raises(TypeError, match=r"RolloutDriver: missing argument 'cell_sort'"):
        ext.RolloutDriver(dict(_zeros(ROLLOUT_OWN), hfwd=None))
    with pytest.raises(TypeError, match=r"RolloutDriver: argument 'hfwd' must be a dict, got int"):
        ext.RolloutDriver(dict(_zeros(ROLLOUT_OWN), hfwd=0))


def test_ext_precision_code_outside_range(ext):
    for fn in (ext.ctrl_fwd, ext.cbf_fwd, ext.cbf_hfwd, ext.cbf_bwd, ext.ctrl_node_bwd, ext.ctrl_edge_bwd):
        with pytest.raises(ValueError, match="precision code 7 outside 0..2"):
            fn(prec=7)
    with pytest.raises(ValueError, match="precision code -1 outside 0..2"):
        ext.ctrl_bwd_step(node={}, edge={}, num_blocks=1, prec=-1, stream=0)
    with pytest.raises(ValueError, match="precision code 3 outside 0..2"):
        ext.node_act_bytes(3)
    with pytest.raises(ValueError, match="precision code 3 outside 0..2"):
        ext.k16_wg_per_cu(3, 0)


NODE_KEYS = ("pooled p_env S s_env dim G A a_env Gn gn_env valid v_env B N wrm o_w1 o_w2 o_w3 o_w4 wvec act_scale "
             "gscale dP dp_env ego partial init chunk stamps").split()


def test_ext_bwd_step_unknown_key_in_the_node_dict(ext):
    node = dict({k: 0 for k in NODE_KEYS}, act_coef=0.0, dt=0.0, sqrt3=0.0)
    with pytest.raises(TypeError, match=r"ctrl_bwd_step node: unexpected argument 'wrm_16'"):
        ext.ctrl_bwd_step(node=dict(node, wrm_16=0), edge={}, num_blocks=1, prec=2, stream=0)
    with pytest.raises(TypeError, match=r"ctrl_bwd_step node: unexpected argument 'a', 'b'"):
        ext.ctrl_bwd_step(node=dict(node, a=1, b=2), edge={}, num_blocks=1, prec=2, stream=0)
    with pytest.raises(TypeError, match=r"ctrl_bwd_step node: argument 'chunk' must be int, got str"):
        ext.ctrl_bwd_step(node=dict(node, chunk="32"), edge={}, num_blocks=1, prec=2, stream=0)
    with pytest.raises(TypeError, match=r"ctrl_bwd_step edge: missing argument 'S'"):
        ext.ctrl_bwd_step(node=node, edge={}, num_blocks=1, prec=2, stream=0)
