"""ctypes binding of libmcgp_hip.so (C ABI: include/mcgp.h).

There is no CPU fallback: if the library is missing it is built with hipcc, and
if that fails, or no HIP device is visible, the error is raised to the caller.
"""
import ctypes as C
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_PKG, 'csrc')
LIB_PATH = os.path.join(_PKG, 'libmcgp_hip.so')

MAX_CARS = 32
MAX_LAPS = 1000
ABI_VERSION = 6

COMPOUNDS = ('SOFT', 'MEDIUM', 'HARD', 'INTERMEDIATE', 'WET')
COMPOUND_ID = {c: i for i, c in enumerate(COMPOUNDS)}
TRACK_ID = {'dry': 0, 'damp': 1, 'wet': 2}


class McgpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f'mcgp error {code}: {msg}')
        self.code = code


class McgpConfig(C.Structure):
    _fields_ = [
        ('total_laps', C.c_int32), ('track_condition', C.c_int32),
        ('pit_loss', C.c_double), ('overtake_delta', C.c_double),
        ('sc_probability', C.c_double), ('vsc_probability', C.c_double),
        ('red_flag_probability', C.c_double), ('drs_delta', C.c_double),
        ('dirty_air_threshold', C.c_double), ('dirty_air_penalty', C.c_double),
        ('comp_pace_delta', C.c_double * 5), ('comp_deg_rate', C.c_double * 5),
        ('comp_optimal_laps', C.c_int32 * 5),
        ('pop_soft_hard', C.c_int32), ('pop_medium_hard', C.c_int32),
        ('deviates', C.c_int32),          # 0: 32-bit deviates (default), 1: the reference's 53-bit / binary64 deviates
    ]


class McgpDrivers(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in
                ('base_pace', 'tire_deg', 'tire_deg_pit', 'variance', 'team_dnf', 'lap_dnf')]


class McgpRaceState(C.Structure):
    """mcgp_race_state: a race after `lap` laps; per-car arrays in driver-index order."""
    _fields_ = [
        ('lap', C.c_int32), ('drs_disabled_until', C.c_int32),
        ('cumulative_time', C.POINTER(C.c_double)), ('last_lap_time', C.POINTER(C.c_double)),
        ('grid_slot', C.POINTER(C.c_uint8)), ('compound', C.POINTER(C.c_uint8)),
        ('used_compounds', C.POINTER(C.c_uint8)),
        ('tire_age', C.POINTER(C.c_int16)), ('retired_lap', C.POINTER(C.c_int16)),
    ]


MAX_PLAN_STOPS = 8
MAX_SCENARIOS = 64
MAX_GAP_EDGES = 63          # include/mcgp.h: MCGP_MAX_GAP_EDGES, MCGP_MAX_GAP_PAIRS
MAX_GAP_PAIRS = 64
MAX_PIT_WINDOWS = 64        # include/mcgp.h: MCGP_MAX_PIT_WINDOWS
STINT_STOPS = 4             # include/mcgp.h: MCGP_STINT_STOPS, MCGP_STINT_SEQ, MCGP_STINT_SEQ_CODES
STINT_SEQ = 4
STINT_SEQ_CODES = 1296
MOVE_DRIVER_CAP = 127       # include/mcgp.h: MCGP_MOVE_DRIVER_CAP, MCGP_MOVE_RACE_CAP
MOVE_RACE_CAP = 1023
MOVE_KINDS = ('made_on_track', 'lost_on_track', 'gained_in_pits', 'lost_in_pits')   # passes_out's kind axis
MAX_CONDITIONS = 64         # include/mcgp.h: MCGP_MAX_CONDITIONS, MCGP_MAX_CONDITION_ATOMS
MAX_CONDITION_ATOMS = 8
# include/mcgp.h: MCGP_FACT_*
(FACT_POSITION, FACT_GRID, FACT_RETIRED_LAP, FACT_AHEAD_BY, FACT_GAINED, FACT_FINISHERS, FACT_RED_FLAGS, FACT_SAFETY_CARS,
 FACT_VSCS) = range(9)


class McgpPitPlan(C.Structure):
    """mcgp_pit_plan: one driver's planned stops in a scenario of mcgp_run_strategies."""
    _fields_ = [
        ('driver', C.c_int32), ('start_compound', C.c_int32), ('start_age', C.c_int32), ('n_stops', C.c_uint32),
        ('stop_lap', C.c_int16 * MAX_PLAN_STOPS), ('stop_compound', C.c_uint8 * MAX_PLAN_STOPS),
    ]


MAX_SCENARIO_PENALTIES = 256                       # include/mcgp.h: MCGP_MAX_SCENARIO_PENALTIES, MCGP_PEN_*
PEN_SERVE_AT_STOP, PEN_AT_FLAG, PEN_ON_LAP = range(3)
PENALTY_KIND = {'serve': PEN_SERVE_AT_STOP, 'flag': PEN_AT_FLAG, 'lap': PEN_ON_LAP}
PENALTY_FATES = ('none', 'served', 'at_flag', 'retired')   # fate_out's last axis


class McgpTimePenalty(C.Structure):
    """mcgp_time_penalty: seconds added to one driver's race in a scenario of mcgp_run_penalties."""
    _fields_ = [('driver', C.c_int32), ('kind', C.c_int32), ('lap', C.c_int32), ('seconds', C.c_double)]


MAX_SCENARIO_EVENTS = 64                           # include/mcgp.h: MCGP_MAX_SCENARIO_EVENTS, MCGP_EVT_*
EVT_NONE, EVT_RED_FLAG, EVT_SAFETY_CAR, EVT_VSC = range(4)
EVENT_KIND = {'none': EVT_NONE, 'red': EVT_RED_FLAG, 'sc': EVT_SAFETY_CAR, 'vsc': EVT_VSC}
EVENT_ROWS = ('red', 'sc', 'vsc')                  # events_out's middle axis


class McgpLapEvent(C.Structure):
    """mcgp_lap_event: the event of laps first_lap..last_lap in a scenario of mcgp_run_events."""
    _fields_ = [('first_lap', C.c_int32), ('last_lap', C.c_int32), ('kind', C.c_int32)]


MAX_SCENARIO_PACES = 64                            # include/mcgp.h: MCGP_MAX_SCENARIO_PACES, MCGP_PACE_*
PACE_LAPS, PACE_UNTIL_STOP = range(2)
MAX_PACE_SECONDS = 60.0


class McgpPaceOffset(C.Structure):
    """mcgp_pace_offset: seconds added to one driver's base pace, on laps or until its next stop, in a scenario of
    mcgp_run_paces."""
    _fields_ = [('driver', C.c_int32), ('kind', C.c_int32), ('first_lap', C.c_int32), ('last_lap', C.c_int32),
                ('seconds', C.c_double)]


MAX_SCENARIO_TRACK_CHANGES = 64                    # include/mcgp.h: MCGP_MAX_SCENARIO_TRACK_CHANGES
MAX_WRONG_TYRE_SECONDS = 60.0
TRACKS = ('dry', 'damp', 'wet')                    # MCGP_DRY .. MCGP_WET_TRACK, by id


GRID_DROP, GRID_PIN, GRID_PIT_LANE = 0, 1, 2       # include/mcgp.h: MCGP_GRID_DROP .. MCGP_GRID_PIT_LANE
MAX_GRID_DROP = 255
MAX_PIT_LANE_SECONDS = 1e6


class McgpGridEdit(C.Structure):
    """mcgp_grid_edit: one driver's drop, pin or pit-lane start in a scenario of mcgp_run_grids."""
    _fields_ = [('driver', C.c_int32), ('kind', C.c_int32), ('value', C.c_int32), ('seconds', C.c_double)]


MAX_SCENARIO_PRIORS = 64                           # include/mcgp.h: MCGP_MAX_SCENARIO_PRIORS, MCGP_PRIOR_*
MAX_PRIOR_EDGES = 15
PRIOR_DRIVER, PRIOR_GROUP = range(2)
MAX_PRIOR_SIGMA = 10.0


class McgpPacePrior(C.Structure):
    """mcgp_pace_prior: the standard deviation of one driver's, or one group's shared, pace error in a scenario of
    mcgp_run_priors."""
    _fields_ = [('kind', C.c_int32), ('driver', C.c_int32), ('members', C.c_uint32), ('pad', C.c_uint32),
                ('sigma', C.c_double)]


class McgpTrackChange(C.Structure):
    """mcgp_track_change: the track condition of laps first_lap..last_lap in a scenario of mcgp_run_weather."""
    _fields_ = [('first_lap', C.c_int32), ('last_lap', C.c_int32), ('condition', C.c_int32)]


class McgpWeatherModel(C.Structure):
    """mcgp_weather_model: seconds a lap on [condition][compound], for one call of mcgp_run_weather."""
    _fields_ = [('wrong_tyre_sec', (C.c_double * 5) * 3)]


class McgpConditionAtom(C.Structure):
    """mcgp_condition_atom: holds iff (lo <= value <= hi) != (negate != 0)."""
    _fields_ = [('fact', C.c_int32), ('a', C.c_int32), ('b', C.c_int32), ('lo', C.c_int32), ('hi', C.c_int32),
                ('negate', C.c_int32)]


class McgpCondition(C.Structure):
    """mcgp_condition: the conjunction of its atoms (none: always true)."""
    _fields_ = [('n_atoms', C.c_uint32), ('atom', McgpConditionAtom * MAX_CONDITION_ATOMS)]


_hash_module = None
_hash_cache = {}            # key -> value; keys carry (path, mtime_ns, size) of every file the value was read from


def _load_source_hash_module():
    global _hash_module
    if _hash_module is None:
        import importlib.util
        spec = importlib.util.spec_from_file_location('_mcgp_source_hash', os.path.join(CSRC, 'source_hash.py'))
        _hash_module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_hash_module)
    return _hash_module


def _sources():
    return _load_source_hash_module().sources()


def _stat_key(paths):
    key = []
    for path in sorted(paths):
        try:
            st = os.stat(path)
            key.append((path, st.st_mtime_ns, st.st_size))
        except OSError:
            key.append((path, None, None))
    return tuple(key)


def source_hash():
    """Identity of the kernel sources in this tree (csrc/source_hash.py): the Makefile compiles the same value into
    libmcgp_hip.so, and profiles under profiles/ are stamped with it.  Cached per process on (path, mtime, size) of
    every hashed file: every rank of a launch asks several times at start-up."""
    key = ('src',) + _stat_key(_sources())
    if key not in _hash_cache:
        for k in [k for k in _hash_cache if k[0] == 'src']:
            del _hash_cache[k]
        _hash_cache[key] = _load_source_hash_module().source_hash()
    return _hash_cache[key]


_MARKER = b'MCGP_BUILD_HASH='


def file_build_hash(path):
    """The source hash a library FILE was compiled from, read from its marker string without loading it
    (None: no such file, or a binary without the marker).  The file (tens of megabytes of kernels) is scanned in
    pieces, not read whole, and the answer is cached per process on (path, mtime, size)."""
    key = ('lib',) + _stat_key([path])
    if key in _hash_cache:
        return _hash_cache[key]
    found = None
    try:
        with open(path, 'rb') as f:
            tail = b''
            while found is None:
                piece = f.read(1 << 20)
                if not piece:
                    break
                blob = tail + piece
                i = blob.find(_MARKER)
                if i >= 0:
                    rest = blob[i + len(_MARKER):]
                    while b'\0' not in rest:                    # the value straddles the end of this piece
                        more = f.read(4096)
                        if not more:
                            break
                        rest += more
                    found = rest.split(b'\0', 1)[0].decode('ascii', 'replace')
                tail = blob[-(len(_MARKER) - 1):]
    except OSError:
        return None
    for k in [k for k in _hash_cache if k[0] == 'lib' and k[1][0] == path]:
        del _hash_cache[k]
    _hash_cache[key] = found
    return found


def _stale():
    """The library is stale unless it carries the hash of the sources beside it (contents, not time stamps: a stale
    binary with a newer mtime is still stale)."""
    return file_build_hash(LIB_PATH) != source_hash()


def build(force=False):
    """Compile csrc/ for gfx950 (hipcc cross-compiles without a GPU).

    One builder per node: an exclusive flock serialises the ranks of a torch.distributed.run launch (the
    first one in builds, the others find the library up to date), make relinks through a temporary file
    renamed into place, and an up-to-date tree is a no-op (make is incremental).  Runs before any HIP call of
    this process.  MCGP_NO_BUILD=1 forbids building (deployments without hipcc, and the staleness test): a stale
    library is then refused instead of rebuilt."""
    if not (force or _stale()):
        return LIB_PATH
    if os.environ.get('MCGP_NO_BUILD') == '1':
        raise McgpError(-1, f'{LIB_PATH} is stale (built from sources {file_build_hash(LIB_PATH)}, the tree is '
                            f'{source_hash()}) and MCGP_NO_BUILD=1 forbids rebuilding it')
    import fcntl
    os.makedirs(os.path.join(CSRC, 'build'), exist_ok=True)
    with open(os.path.join(CSRC, 'build', '.lock'), 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if force or _stale():
                subprocess.check_call(['make', '-C', CSRC, '-s'] + (['-B'] if force else []))
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    if _stale():
        raise McgpError(-1, f'{LIB_PATH} still carries source hash {file_build_hash(LIB_PATH)} after make; the tree '
                            f'is {source_hash()}')
    return LIB_PATH


def hip_runtimes_mapped():
    """Paths of the libamdhip64 copies mapped into this process (one in a healthy process)."""
    paths = set()
    try:
        with open('/proc/self/maps') as f:
            for line in f:
                if 'libamdhip64' in line:
                    paths.add(line.split(None, 5)[-1].strip())
    except OSError:
        pass
    return sorted(paths)


def _bind_hip_runtime():
    """Make libmcgp_hip.so and PyTorch share ONE HIP runtime, whichever is loaded first.

    libmcgp_hip.so needs `libamdhip64.so.7` (found in /opt/rocm through its RUNPATH); PyTorch-ROCm ships its own
    copy and asks for it as `libamdhip64.so`, a name the loader does not match against an already mapped
    /opt/rocm copy.  Library first, torch second therefore maps two runtimes, and the second one finds no GPU
    ("No HIP GPUs are available"); a hipStream_t of one handed to the other is undefined behaviour.  So when a
    torch installation is present (located without importing it) and no runtime is mapped yet, map ITS copy
    globally first: the library's NEEDED entry then binds to it by SONAME, and a later `import torch` finds
    the same file.  MCGP_HIP_RUNTIME=system skips this (torch-free deployments), or names a libamdhip64 to use."""
    if hip_runtimes_mapped():
        return
    choice = os.environ.get('MCGP_HIP_RUNTIME', '')
    if choice == 'system':
        return
    cand = choice
    if not cand:
        import importlib.util
        try:
            spec = importlib.util.find_spec('torch')
        except (ImportError, ValueError):
            spec = None
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), 'lib', 'libamdhip64.so')
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def assert_single_hip_runtime():
    """Raise if this process has ended up with two HIP runtimes (library loaded against one, torch.cuda on another)."""
    mapped = hip_runtimes_mapped()
    if len(mapped) > 1:
        raise McgpError(-3, 'two HIP runtimes are mapped into this process (' + ', '.join(mapped) + '): '
                        'streams and device state cannot be shared between them; import torch before '
                        'loading the library or set MCGP_HIP_RUNTIME')


_lib = None

EXPORTS = ('mcgp_abi_version', 'mcgp_build_hash', 'mcgp_run_batch', 'mcgp_device_count', 'mcgp_last_error', 'mcgp_run', 'mcgp_run_device',
           'mcgp_simulate_race', 'mcgp_grid_probs', 'mcgp_run_from_ratings', 'mcgp_last_kernel_ms',
           'mcgp_stream_kernel_ms', 'mcgp_elo_season',
           'mcgp_last_launch_info', 'mcgp_last_kernel_name', 'mcgp_run_championship', 'mcgp_run_matchups',
           'mcgp_run_from_state', 'mcgp_run_trace', 'mcgp_run_strategies', 'mcgp_run_gaps', 'mcgp_run_conditions',
           'mcgp_run_championship_rounds', 'mcgp_run_stints', 'mcgp_run_moves', 'mcgp_run_championship_bonus',
           'mcgp_run_penalties', 'mcgp_run_events', 'mcgp_run_championship_live', 'mcgp_run_paces',
           'mcgp_run_combined', 'mcgp_run_weather', 'mcgp_run_grids', 'mcgp_run_pit_windows',
           'mcgp_run_priors')


# mcgp_run_gaps(cfg, drv, grid_probs, state, n, n_edges, edges, n_pairs, pairs, n_sims, sim_offset, seed, device, hist_out,
# lap_gap_out, lead_out, pair_out)
GAPS_ARGTYPES = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), C.POINTER(C.c_double), C.POINTER(McgpRaceState),
                 C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_uint8), C.c_uint64, C.c_uint64,
                 C.c_uint64, C.c_int32] + [C.POINTER(C.c_uint64)] * 4

# mcgp_run_pit_windows(cfg, drv, grid_probs, state, n, n_edges, edges, n_windows, window_drivers, window_losses, n_sims,
# sim_offset, seed, device, hist_out, rejoin_out, lost_out, ahead_out, gap_ahead_out, gap_behind_out)
PIT_WINDOWS_ARGTYPES = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), C.POINTER(C.c_double), C.POINTER(McgpRaceState),
                        C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_uint8),
                        C.POINTER(C.c_double), C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32] + [C.POINTER(C.c_uint64)] * 6

# mcgp_run_conditions(cfg, drv, grid_probs, state, n, n_conditions, conditions, n_sims, sim_offset, seed, device, hist_out,
# count_out, cond_hist_out)
CONDITIONS_ARGTYPES = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), C.POINTER(C.c_double), C.POINTER(McgpRaceState),
                       C.c_uint32, C.c_uint32, C.POINTER(McgpCondition), C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32] \
    + [C.POINTER(C.c_uint64)] * 3

# mcgp_run_stints(cfg, drv, grid_probs, state, n, n_sims, sim_offset, seed, device, hist_out, stop_lap_out, stops_pos_out,
# seq_out)
STINTS_ARGTYPES = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), C.POINTER(C.c_double), C.POINTER(McgpRaceState),
                   C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32] + [C.POINTER(C.c_uint64)] * 4

# mcgp_run_moves(cfg, drv, grid_probs, state, n, n_sims, sim_offset, seed, device, hist_out, grid_fin_out, start_gain_out,
# passes_out, race_passes_out, lap_passes_out, pair_passes_out)
MOVES_ARGTYPES = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), C.POINTER(C.c_double), C.POINTER(McgpRaceState),
                  C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32] + [C.POINTER(C.c_uint64)] * 7


def lib():
    """Load the library (building it if the sources are newer); raises if impossible."""
    global _lib
    if _lib is None:
        # another build of the library (diagnostic builds: the ablation records were made by tools/ablate.sh as of commit 355385d)
        path = os.environ.get('MCGP_LIB')
        if not path:
            build()
            path = LIB_PATH
        _bind_hip_runtime()
        L = C.CDLL(path)
        assert_single_hip_runtime()
        if hasattr(L, 'mcgp_build_hash'):
            L.mcgp_build_hash.restype = C.c_char_p
        if not os.environ.get('MCGP_LIB'):
            # the binary that is MAPPED must be the one whose file was checked (a rebuild renames a new file into place)
            loaded = L.mcgp_build_hash().decode() if hasattr(L, 'mcgp_build_hash') else None
            if loaded != source_hash():
                raise McgpError(-1, f'{path} was compiled from sources {loaded}, the tree is {source_hash()}: refusing '
                                    'to run a stale kernel')
        L.mcgp_abi_version.restype = C.c_int32
        L.mcgp_device_count.restype = C.c_int32
        L.mcgp_last_error.restype = C.c_char_p
        dp = C.POINTER(C.c_double)
        L.mcgp_run.restype = C.c_int32
        L.mcgp_run.argtypes = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), dp, C.c_uint32, C.c_uint64,
                               C.c_uint64, C.c_uint64, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)]
        if hasattr(L, 'mcgp_run_batch'):
            L.mcgp_run_batch.restype = C.c_int32
            L.mcgp_run_batch.argtypes = [C.c_uint32, C.POINTER(McgpConfig), C.POINTER(McgpDrivers), C.POINTER(dp), C.c_uint32,
                                         C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int32,
                                         C.POINTER(C.c_uint64)]
        L.mcgp_run_device.restype = C.c_int32
        L.mcgp_run_device.argtypes = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), dp, C.c_uint32, C.c_uint64,
                                      C.c_uint64, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcgp_simulate_race.restype = C.c_int32
        L.mcgp_simulate_race.argtypes = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), C.POINTER(C.c_uint8),
                                         C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32, C.POINTER(C.c_uint8)]
        ip = C.POINTER(C.c_int32)
        missing = [f for f in EXPORTS if not hasattr(L, f)]
        if missing and not os.environ.get('MCGP_LIB'):          # diagnostic builds of older sources may lack entry points
            raise McgpError(-1, f'{path} does not export {missing}')
        if 'mcgp_grid_probs' not in missing:
            L.mcgp_grid_probs.restype = C.c_int32
            L.mcgp_grid_probs.argtypes = [dp, dp, dp, dp, ip, C.c_uint32, C.c_int32, dp]
            L.mcgp_run_from_ratings.restype = C.c_int32
            L.mcgp_run_from_ratings.argtypes = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), dp, dp, dp, dp, ip,
                                                C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32,
                                                C.POINTER(C.c_uint64), dp]
        if 'mcgp_elo_season' not in missing:
            L.mcgp_elo_season.restype = C.c_int32
            L.mcgp_elo_season.argtypes = [C.c_uint32, C.c_uint32, ip, dp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), dp,
                                          dp, dp, C.c_int32]
        if 'mcgp_run_championship' not in missing:
            u64p = C.POINTER(C.c_uint64)
            L.mcgp_run_championship.restype = C.c_int32
            L.mcgp_run_championship.argtypes = [C.c_uint32, C.POINTER(McgpConfig), C.POINTER(McgpDrivers), C.POINTER(dp),
                                                C.c_uint32, C.c_uint64, C.c_uint64, u64p, ip, C.POINTER(C.c_uint8), ip, ip,
                                                ip, C.c_uint32, C.c_int32, u64p, u64p, u64p, u64p]
        if 'mcgp_run_championship_rounds' not in missing:
            # mcgp_run_championship's arguments, then round_hist, contend_out, secure_out and the teams' three
            L.mcgp_run_championship_rounds.restype = C.c_int32
            L.mcgp_run_championship_rounds.argtypes = L.mcgp_run_championship.argtypes + [C.POINTER(C.c_uint64)] * 6
        if 'mcgp_run_championship_bonus' not in missing and 'mcgp_run_championship_rounds' not in missing:
            # mcgp_run_championship_rounds' arguments, then bonus_points, bonus_within, bonus_hist, fastest_hist
            L.mcgp_run_championship_bonus.restype = C.c_int32
            L.mcgp_run_championship_bonus.argtypes = L.mcgp_run_championship_rounds.argtypes + [ip, ip] \
                + [C.POINTER(C.c_uint64)] * 2
        if 'mcgp_run_championship_live' not in missing and 'mcgp_run_championship_bonus' not in missing \
                and 'mcgp_run_championship_rounds' not in missing:
            # mcgp_run_championship_bonus' arguments, then state0, given_race, title_given_out
            L.mcgp_run_championship_live.restype = C.c_int32
            L.mcgp_run_championship_live.argtypes = L.mcgp_run_championship_bonus.argtypes \
                + [C.POINTER(McgpRaceState), C.c_int32, C.POINTER(C.c_uint64)]
        if 'mcgp_run_matchups' not in missing:
            u64p = C.POINTER(C.c_uint64)
            L.mcgp_run_matchups.restype = C.c_int32
            L.mcgp_run_matchups.argtypes = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), dp, C.c_uint32, C.c_uint64,
                                            C.c_uint64, C.c_uint64, C.c_int32, u64p, u64p, u64p]
        if 'mcgp_run_from_state' not in missing:
            L.mcgp_run_from_state.restype = C.c_int32
            L.mcgp_run_from_state.argtypes = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), C.c_uint32, C.c_uint32,
                                              C.POINTER(McgpRaceState), C.c_uint64, C.POINTER(C.c_uint64), C.c_uint64,
                                              C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)]
        if 'mcgp_run_trace' not in missing:
            u64p = C.POINTER(C.c_uint64)
            L.mcgp_run_trace.restype = C.c_int32
            L.mcgp_run_trace.argtypes = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), dp, C.c_uint32, C.c_uint64,
                                         C.c_uint64, C.c_uint64, C.c_int32, u64p, u64p, u64p, u64p, u64p, u64p]
        if 'mcgp_run_strategies' not in missing:
            u64p = C.POINTER(C.c_uint64)
            L.mcgp_run_strategies.restype = C.c_int32
            L.mcgp_run_strategies.argtypes = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), dp, C.POINTER(McgpRaceState),
                                              C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(McgpPitPlan),
                                              C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, u64p, u64p,
                                              C.POINTER(C.c_uint8)]
        if 'mcgp_run_penalties' not in missing:
            u64p = C.POINTER(C.c_uint64)
            L.mcgp_run_penalties.restype = C.c_int32
            L.mcgp_run_penalties.argtypes = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), dp, C.POINTER(McgpRaceState),
                                             C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(McgpPitPlan),
                                             C.POINTER(C.c_uint32), C.POINTER(McgpTimePenalty), C.c_uint64, C.c_uint64,
                                             C.c_uint64, C.c_int32, u64p, u64p, u64p, C.POINTER(C.c_uint8)]
        if 'mcgp_run_events' not in missing:
            u64p = C.POINTER(C.c_uint64)
            L.mcgp_run_events.restype = C.c_int32
            L.mcgp_run_events.argtypes = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), dp, C.POINTER(McgpRaceState),
                                          C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(McgpPitPlan),
                                          C.POINTER(C.c_uint32), C.POINTER(McgpLapEvent), C.c_uint64, C.c_uint64,
                                          C.c_uint64, C.c_int32, u64p, u64p, u64p, C.POINTER(C.c_uint8)]
        if 'mcgp_run_paces' not in missing:
            u64p = C.POINTER(C.c_uint64)
            L.mcgp_run_paces.restype = C.c_int32
            L.mcgp_run_paces.argtypes = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), dp, C.POINTER(McgpRaceState),
                                         C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(McgpPitPlan),
                                         C.POINTER(C.c_uint32), C.POINTER(McgpPaceOffset), C.c_uint64, C.c_uint64,
                                         C.c_uint64, C.c_int32, u64p, u64p, u64p, C.POINTER(C.c_uint8)]
        if 'mcgp_run_combined' not in missing:
            # the plans, then (count, items) of the penalties, the events and the offsets, any pair of which may be NULL;
            # hist, delta, fate, events, carried, orders
            u64p = C.POINTER(C.c_uint64)
            L.mcgp_run_combined.restype = C.c_int32
            L.mcgp_run_combined.argtypes = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), dp, C.POINTER(McgpRaceState),
                                            C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(McgpPitPlan),
                                            C.POINTER(C.c_uint32), C.POINTER(McgpTimePenalty),
                                            C.POINTER(C.c_uint32), C.POINTER(McgpLapEvent),
                                            C.POINTER(C.c_uint32), C.POINTER(McgpPaceOffset), C.c_uint64, C.c_uint64,
                                            C.c_uint64, C.c_int32, u64p, u64p, u64p, u64p, u64p, C.POINTER(C.c_uint8)]
        if 'mcgp_run_weather' not in missing:
            # the plans, (count, changes), the call's model; hist, delta, wrong_laps, orders
            u64p = C.POINTER(C.c_uint64)
            L.mcgp_run_weather.restype = C.c_int32
            L.mcgp_run_weather.argtypes = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), dp, C.POINTER(McgpRaceState),
                                           C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(McgpPitPlan),
                                           C.POINTER(C.c_uint32), C.POINTER(McgpTrackChange),
                                           C.POINTER(McgpWeatherModel), C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32,
                                           u64p, u64p, u64p, C.POINTER(C.c_uint8)]
        if 'mcgp_run_grids' not in missing:
            # no state; the plans, (count, edits); hist, delta, start, gain, orders
            u64p = C.POINTER(C.c_uint64)
            L.mcgp_run_grids.restype = C.c_int32
            L.mcgp_run_grids.argtypes = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), dp, C.c_uint32, C.c_uint32,
                                         C.POINTER(C.c_uint32), C.POINTER(McgpPitPlan), C.POINTER(C.c_uint32),
                                         C.POINTER(McgpGridEdit), C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32,
                                         u64p, u64p, u64p, u64p, C.POINTER(C.c_uint8)]
        if 'mcgp_run_priors' not in missing:
            # the plans, (count, items), (n_edges, edges); hist, delta, draws, offsets, orders
            u64p = C.POINTER(C.c_uint64)
            L.mcgp_run_priors.restype = C.c_int32
            L.mcgp_run_priors.argtypes = [C.POINTER(McgpConfig), C.POINTER(McgpDrivers), dp, C.POINTER(McgpRaceState),
                                          C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(McgpPitPlan),
                                          C.POINTER(C.c_uint32), C.POINTER(McgpPacePrior), C.c_uint32, dp, C.c_uint64,
                                          C.c_uint64, C.c_uint64, C.c_int32, u64p, u64p, u64p, C.POINTER(C.c_float),
                                          C.POINTER(C.c_uint8)]
        if 'mcgp_run_gaps' not in missing:
            L.mcgp_run_gaps.restype = C.c_int32
            L.mcgp_run_gaps.argtypes = GAPS_ARGTYPES
        if 'mcgp_run_pit_windows' not in missing:
            L.mcgp_run_pit_windows.restype = C.c_int32
            L.mcgp_run_pit_windows.argtypes = PIT_WINDOWS_ARGTYPES
        if 'mcgp_run_conditions' not in missing:
            L.mcgp_run_conditions.restype = C.c_int32
            L.mcgp_run_conditions.argtypes = CONDITIONS_ARGTYPES
        if 'mcgp_run_stints' not in missing:
            L.mcgp_run_stints.restype = C.c_int32
            L.mcgp_run_stints.argtypes = STINTS_ARGTYPES
        if 'mcgp_run_moves' not in missing:
            L.mcgp_run_moves.restype = C.c_int32
            L.mcgp_run_moves.argtypes = MOVES_ARGTYPES
        L.mcgp_last_kernel_ms.restype = C.c_int32
        L.mcgp_last_kernel_ms.argtypes = [C.c_int32, C.POINTER(C.c_float)]
        if 'mcgp_stream_kernel_ms' not in missing:
            L.mcgp_stream_kernel_ms.restype = C.c_int32
            L.mcgp_stream_kernel_ms.argtypes = [C.c_int32, C.c_void_p, C.POINTER(C.c_float)]
        L.mcgp_last_kernel_name.restype = C.c_char_p
        L.mcgp_last_kernel_name.argtypes = [C.c_int32]
        L.mcgp_last_launch_info.restype = C.c_int32
        L.mcgp_last_launch_info.argtypes = [C.c_int32] + [C.POINTER(C.c_uint32)] * 3
        if L.mcgp_abi_version() != ABI_VERSION:
            raise McgpError(-1, f'ABI version {L.mcgp_abi_version()} != {ABI_VERSION}')
        _lib = L
    return _lib


def build_hash():
    """Source hash compiled into the library this process has loaded (mcgp_build_hash())."""
    L = lib()
    return L.mcgp_build_hash().decode() if hasattr(L, 'mcgp_build_hash') else None


def check(rc):
    if rc != 0:
        raise McgpError(rc, lib().mcgp_last_error().decode('utf-8', 'replace'))
