//! rustronomy-watershed's public interface (v0.4.1) with the transforms running on an AMD MI355X through the
//! C ABI of include/ws_hip.h.  "lib.rs:N" = line N of the reference's src/lib.rs.
//!
//! Same names, signatures and error behaviour as the reference: `TransformBuilder` (lib.rs:908-1047), `BuildErr`
//! (lib.rs:1051-1065), `HookCtx` (lib.rs:844-862), `Watershed<T>` (lib.rs:1206-1238), `WatershedUtils`
//! (lib.rs:1069-1198), `MergingWatershed` / `SegmentingWatershed`.  Deviations, all documented in ws_hip.h:
//! the tie-break where lakes meet is the first coloured neighbour in down, right, left, up order (a legal outcome
//! of lib.rs:249-253); `SegmentingWatershed::transform` returns the labels after the last level instead of
//! panicking (lib.rs:1821); merged-lake ids are the smallest seed colour of the lake.  Out of scope here: the
//! `plots`, `progress`, `debug` and `jemalloc` features.
//!
//! This crate is source only in this repository: its build image has no Rust toolchain.
mod hip_ffi;
mod shim;

use ndarray as nd;
use num_traits::{Num, ToPrimitive};
use std::os::raw::{c_int, c_void};

pub const UNCOLOURED: usize = 0; // lib.rs:138
pub const NORMAL_MAX: u8 = 254; // lib.rs:139
pub const ALWAYS_FILL: u8 = 0; // lib.rs:140
pub const NEVER_FILL: u8 = 255; // lib.rs:141

pub mod prelude {
    pub use crate::{MergingWatershed, SegmentingWatershed, TransformBuilder, Watershed, WatershedUtils};
}

/// lib.rs:844-850
#[derive(Clone)]
pub struct HookCtx<'a> {
    pub water_level: u8,
    pub max_water_level: u8,
    pub image: nd::ArrayView2<'a, u8>,
    pub colours: nd::ArrayView2<'a, usize>,
    pub seeds: &'a [(usize, (usize, usize))],
}

/// lib.rs:1051-1065
#[derive(Debug, Clone)]
pub enum BuildErr {
    MaxToHigh(u8),
    MaxToLow(u8),
}

impl std::error::Error for BuildErr {}
impl std::fmt::Display for BuildErr {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        match self {
            BuildErr::MaxToHigh(v) => {
                write!(f, "Maximum water level set to {v}, which is higher than the maximum allowed value {NORMAL_MAX}")
            }
            // the reference's message names NEVER_FILL here too (lib.rs:1062)
            BuildErr::MaxToLow(v) => {
                write!(f, "Maximum water level set to {v}, which is lower than the minimum allowed value {NEVER_FILL}")
            }
        }
    }
}

/// The options every transform struct carries (the reference's private fields, lib.rs:1297-1311, 1609-1621).
#[derive(Clone, Copy)]
struct Options {
    max_water_level: u8,
    edge_correction: bool,
    seed_shift: bool,
}

impl Options {
    fn ffi(&self) -> hip_ffi::ws_options {
        hip_ffi::ws_options {
            max_water_level: self.max_water_level,
            edge_correction: self.edge_correction as u8,
            engine: 0,   // WS_ENGINE_AUTO
            tie_rule: 0, // WS_TIE_FIRST_DRLU
            seed_shift: self.seed_shift as u8,
            reserved: [0; 3],
        }
    }
    /// shape of every label plane the transform hands out (lib.rs:1640-1666: outputs stay padded)
    fn plane(&self, h: usize, w: usize) -> (usize, usize) {
        let e = if self.edge_correction { 2 } else { 0 };
        (h + e, w + e)
    }
}

/// lib.rs:908-923
#[derive(Clone)]
pub struct TransformBuilder<T = ()> {
    opt: Options,
    wlvl_hook: Option<fn(HookCtx) -> T>,
}

impl Default for TransformBuilder<()> {
    fn default() -> Self {
        TransformBuilder::new()
    }
}

impl<T> TransformBuilder<T> {
    /// lib.rs:936-946: max level 254, no edge correction, no hook
    pub const fn new() -> Self {
        TransformBuilder {
            opt: Options { max_water_level: NORMAL_MAX, edge_correction: false, seed_shift: false },
            wlvl_hook: None,
        }
    }
    /// lib.rs:950
    pub const fn set_max_water_lvl(mut self, max_water_lvl: u8) -> Self {
        self.opt.max_water_level = max_water_lvl;
        self
    }
    /// lib.rs:958.  No padded image copy is made on the device: the ring of zeros is virtual.
    pub const fn enable_edge_correction(mut self) -> Self {
        self.opt.edge_correction = true;
        self
    }
    /// lib.rs:967
    pub const fn set_wlvl_hook(mut self, hook: fn(HookCtx) -> T) -> Self {
        self.wlvl_hook = Some(hook);
        self
    }
    /// Not in the reference (`ws_options.seed_shift`): with edge correction, move every seed by (+1, +1) onto the
    /// pixel it was found at, instead of indexing the padded plane with the caller's coordinates (lib.rs:1675-1677).
    pub const fn shift_seeds_into_padded_plane(mut self) -> Self {
        self.opt.seed_shift = true;
        self
    }

    fn validate(&self) -> Result<(), BuildErr> {
        // lib.rs:999-1004, 1026-1030; ws_options_validate returns the same two errors to non-Rust callers
        if self.opt.max_water_level > NORMAL_MAX {
            Err(BuildErr::MaxToHigh(self.opt.max_water_level))
        } else if self.opt.max_water_level <= ALWAYS_FILL {
            Err(BuildErr::MaxToLow(self.opt.max_water_level))
        } else {
            Ok(())
        }
    }
    /// lib.rs:998-1020
    pub fn build_merging(self) -> Result<MergingWatershed<T>, BuildErr> {
        self.validate()?;
        Ok(MergingWatershed { opt: self.opt, wlvl_hook: self.wlvl_hook })
    }
    /// lib.rs:1024-1046
    pub fn build_segmenting(self) -> Result<SegmentingWatershed<T>, BuildErr> {
        self.validate()?;
        Ok(SegmentingWatershed { opt: self.opt, wlvl_hook: self.wlvl_hook })
    }
}

/// lib.rs:1069-1198
pub trait WatershedUtils {
    /// lib.rs:1081-1087
    fn pre_processor<T, D>(&self, img: nd::ArrayView<T, D>) -> nd::Array<u8, D>
    where
        T: Num + Copy + ToPrimitive + PartialOrd + 'static,
        D: nd::Dimension,
    {
        self.pre_processor_with_max::<NORMAL_MAX, T, D>(img)
    }

    /// lib.rs:1134-1173.  Element types the ABI lists (f32, f64, i32, u16, i16, u8) are quantised on the GPU with
    /// the reference's arithmetic (zero-seeded min / max folds, f64, `is_normal` quirks: NaN, -inf, subnormals and
    /// exact 0 -> NEVER_FILL, +inf -> ALWAYS_FILL); any other `T` goes through f64 on the host first, which is
    /// what the reference's `to_f64()` does per element anyway.
    fn pre_processor_with_max<const MAX: u8, T, D>(&self, img: nd::ArrayView<T, D>) -> nd::Array<u8, D>
    where
        T: Num + Copy + ToPrimitive + PartialOrd + 'static,
        D: nd::Dimension,
    {
        assert!(MAX < NEVER_FILL); // lib.rs:1143
        assert!(MAX > ALWAYS_FILL); // lib.rs:1144
        use std::any::TypeId;
        let t = TypeId::of::<T>();
        let dtype = [
            (TypeId::of::<f32>(), hip_ffi::WS_F32),
            (TypeId::of::<f64>(), hip_ffi::WS_F64),
            (TypeId::of::<i32>(), hip_ffi::WS_I32),
            (TypeId::of::<u16>(), hip_ffi::WS_U16),
            (TypeId::of::<i16>(), hip_ffi::WS_I16),
            (TypeId::of::<u8>(), hip_ffi::WS_U8),
        ]
        .iter()
        .find(|(id, _)| *id == t)
        .map(|&(_, d)| d);
        let mut out = nd::Array::<u8, D>::zeros(img.raw_dim());
        let n = img.len();
        let std_img = img.as_standard_layout();
        let out_ptr = out.as_slice_mut().expect("fresh array is contiguous").as_mut_ptr();
        shim::with_ctx(|ctx| unsafe {
            let rc = match dtype {
                Some(d) => hip_ffi::ws_pre_processor(ctx, std_img.as_ptr() as *const c_void, d, n, MAX, out_ptr),
                None => {
                    let wide: Vec<f64> = std_img.iter().map(|x| x.to_f64().unwrap()).collect();
                    hip_ffi::ws_pre_processor(ctx, wide.as_ptr() as *const c_void, hip_ffi::WS_F64, n, MAX, out_ptr)
                }
            };
            shim::check(ctx, rc, "ws_pre_processor");
        });
        out
    }

    /// lib.rs:1178-1197: strict 8-neighbour local MAXIMA of the interior (as the reference's code does, whatever
    /// its name says), in row-major order.
    fn find_local_minima(&self, img: nd::ArrayView2<u8>) -> Vec<(usize, usize)> {
        let (h, w) = img.dim();
        if h < 3 || w < 3 {
            return Vec::new(); // no 3x3 window (lib.rs:1183)
        }
        let (std_img, stride) = shim::standard(&img);
        // at most one strict maximum per 2x2 block
        let cap = ((h - 1) / 2 + 1) * ((w - 1) / 2 + 1);
        let mut rc_pairs = vec![0u64; 2 * cap];
        let mut n = 0usize;
        shim::with_ctx(|ctx| unsafe {
            let rc = hip_ffi::ws_find_local_minima(ctx, std_img.as_ptr(), h, w, stride, rc_pairs.as_mut_ptr(), cap, &mut n);
            shim::check(ctx, rc, "ws_find_local_minima");
        });
        rc_pairs[..2 * n].chunks_exact(2).map(|p| (p[0] as usize, p[1] as usize)).collect()
    }

    /// Not in the reference: `pre_processor_with_max::<MAX>` of every slice `cube.index_axis(axis, k)` of a cube as one call
    /// (tests/integration.rs:267-290 slice a FITS cube along its LAST axis and normalise one slice after the other).  The view
    /// goes to the engine with its own strides -- a channel-last cube needs no copy into planes -- and the result is the
    /// standard-layout `(n_slices, h, w)` cube the `*_cube` methods take.  Element types outside the ABI's list, and views
    /// with a negative stride, are first copied (as f64 / into standard layout).
    fn pre_processor_cube_with_max<const MAX: u8, T>(&self, cube: nd::ArrayView3<T>, axis: nd::Axis) -> nd::Array3<u8>
    where
        T: Num + Copy + ToPrimitive + PartialOrd + 'static,
    {
        assert!(MAX < NEVER_FILL); // lib.rs:1143
        assert!(MAX > ALWAYS_FILL); // lib.rs:1144
        assert!(axis.index() < 3);
        use std::any::TypeId;
        let t = TypeId::of::<T>();
        let dtype = [
            (TypeId::of::<f32>(), hip_ffi::WS_F32),
            (TypeId::of::<f64>(), hip_ffi::WS_F64),
            (TypeId::of::<i32>(), hip_ffi::WS_I32),
            (TypeId::of::<u16>(), hip_ffi::WS_U16),
            (TypeId::of::<i16>(), hip_ffi::WS_I16),
            (TypeId::of::<u8>(), hip_ffi::WS_U8),
        ]
        .iter()
        .find(|(id, _)| *id == t)
        .map(|&(_, d)| d);
        let others: Vec<usize> = (0..3).filter(|&a| a != axis.index()).collect();
        let view = cube.permuted_axes([axis.index(), others[0], others[1]]);
        let (n, h, w) = view.dim();
        let mut out = nd::Array3::<u8>::zeros((n, h, w));
        let out_ptr = out.as_slice_mut().expect("fresh array is contiguous").as_mut_ptr();
        let mut failed = 0usize;
        let run = |ptr: *const c_void, d: c_int, st: [usize; 3], failed: &mut usize| {
            shim::with_ctx(|ctx| unsafe {
                let rc = hip_ffi::ws_pre_processor_batch(ctx, ptr, d, n, h, w, st[0], st[1], st[2], MAX, out_ptr, std::ptr::null_mut(), failed);
                shim::check(ctx, rc, "ws_pre_processor_batch");
            })
        };
        let strided = view.strides().iter().all(|&s| s >= 0);
        match dtype {
            Some(d) if strided => {
                let st = view.strides();
                run(view.as_ptr() as *const c_void, d, [st[0] as usize, st[1] as usize, st[2] as usize], &mut failed)
            }
            Some(d) => {
                let std_view = view.as_standard_layout();
                run(std_view.as_ptr() as *const c_void, d, [h * w, w, 1], &mut failed)
            }
            None => {
                let wide: Vec<f64> = view.iter().map(|x| x.to_f64().unwrap()).collect();
                run(wide.as_ptr() as *const c_void, hip_ffi::WS_F64, [h * w, w, 1], &mut failed)
            }
        }
        out
    }

    /// Not in the reference: `find_local_minima` of every slice of a standard-layout `(n_slices, h, w)` cube as one call.  Returns
    /// the slices' lists back to back and `n_slices + 1` offsets: slice `k`'s seeds are `seeds[offsets[k]..offsets[k + 1]]`.
    fn find_local_minima_cube(&self, cube: nd::ArrayView3<u8>) -> (Vec<(usize, usize)>, Vec<usize>) {
        let (n, h, w) = cube.dim();
        let mut offsets = vec![0usize; n + 1];
        if n == 0 || h < 3 || w < 3 {
            return (Vec::new(), offsets);
        }
        let std_cube = cube.as_standard_layout();
        let cap = ((h - 1) / 2 + 1) * ((w - 1) / 2 + 1) * n;
        let mut rc_pairs = vec![0u64; 2 * cap];
        let mut found = 0usize;
        shim::with_ctx(|ctx| unsafe {
            let rc = hip_ffi::ws_find_local_minima_batch(ctx, std_cube.as_ptr(), n, h, w, w, h * w, rc_pairs.as_mut_ptr(), cap,
                                                         offsets.as_mut_ptr(), &mut found);
            shim::check(ctx, rc, "ws_find_local_minima_batch");
        });
        (rc_pairs[..2 * found].chunks_exact(2).map(|p| (p[0] as usize, p[1] as usize)).collect(), offsets)
    }
}

impl<T> WatershedUtils for MergingWatershed<T> {}
impl<T> WatershedUtils for SegmentingWatershed<T> {}

/// lib.rs:1206-1238
pub trait Watershed<T = ()> {
    fn transform(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)]) -> nd::Array2<usize>;
    fn transform_with_hook(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)]) -> Vec<T>;
    fn transform_to_list(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)]) -> Vec<(u8, Vec<usize>)>;
    fn transform_history(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)]) -> Vec<(u8, nd::Array2<usize>)>;
}

/// lib.rs:1297-1311
pub struct MergingWatershed<T = ()> {
    opt: Options,
    wlvl_hook: Option<fn(HookCtx) -> T>,
}

/// lib.rs:1609-1621
pub struct SegmentingWatershed<T = ()> {
    opt: Options,
    wlvl_hook: Option<fn(HookCtx) -> T>,
}

// ---- the three ABI call shapes both transforms share ------------------------------------------------------------

/// `ws_segment_with_hook` / `ws_merge_with_hook`: lib.rs:1638-1808 / 1328-1522.  The whole transform runs even
/// without a hook (the reference does the same and returns an empty Vec, lib.rs:1796-1807).
fn run_with_hook<U>(merging: bool, opt: &Options, hook: Option<fn(HookCtx) -> U>, input: nd::ArrayView2<u8>,
                    seeds: &[(usize, usize)], final_labels: Option<&mut nd::Array2<usize>>) -> Vec<U> {
    let (h, w) = input.dim();
    let (std_img, stride) = shim::standard(&input);
    let packed = shim::pack_seeds(seeds);
    let colours = shim::seed_colours(seeds);
    let o = opt.ffi();
    let out_ptr = match final_labels {
        Some(a) => {
            assert_eq!(a.dim(), opt.plane(h, w));
            a.as_slice_mut().expect("standard layout").as_mut_ptr() as *mut u64
        }
        None => std::ptr::null_mut(),
    };
    match hook {
        Some(f) => {
            let mut st = shim::HookState { hook: f, seeds: &colours, results: Vec::with_capacity(opt.max_water_level as usize + 1) };
            let user = &mut st as *mut _ as *mut c_void;
            let cb: hip_ffi::ws_level_cb = Some(shim::trampoline::<U>);
            shim::with_ctx(|ctx| unsafe {
                let rc = if merging {
                    hip_ffi::ws_merge_with_hook(ctx, std_img.as_ptr(), h, w, stride, packed.as_ptr(), seeds.len(), &o, cb, user, out_ptr)
                } else {
                    hip_ffi::ws_segment_with_hook(ctx, std_img.as_ptr(), h, w, stride, packed.as_ptr(), seeds.len(), &o, cb, user, out_ptr)
                };
                shim::check(ctx, rc, "transform_with_hook");
            });
            st.results
        }
        None => {
            let user = std::ptr::null_mut();
            shim::with_ctx(|ctx| unsafe {
                let rc = if merging {
                    hip_ffi::ws_merge_with_hook(ctx, std_img.as_ptr(), h, w, stride, packed.as_ptr(), seeds.len(), &o, None, user, out_ptr)
                } else {
                    hip_ffi::ws_segment_with_hook(ctx, std_img.as_ptr(), h, w, stride, packed.as_ptr(), seeds.len(), &o, None, user, out_ptr)
                };
                shim::check(ctx, rc, "transform_with_hook");
            });
            Vec::new()
        }
    }
}

/// `ws_transform_to_list` + the dense expansion the reference's return type asks for: per level a `Vec<usize>` of
/// length pixels + 1 with `v[c]` = area of lake `c`, `v[0]` = uncoloured pixels (lib.rs:628-635, 1551-1561,
/// 1837-1847).  The engine returns (colour, area) records; the records of a level are sorted by colour.
fn run_to_list(merging: bool, opt: &Options, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)]) -> Vec<(u8, Vec<usize>)> {
    let (h, w) = input.dim();
    let (ph, pw) = opt.plane(h, w);
    let (std_img, stride) = shim::standard(&input);
    let packed = shim::pack_seeds(seeds);
    let o = opt.ffi();
    let levels = opt.max_water_level as usize + 1;
    let mut offsets = vec![0u64; levels + 1];
    let mut uncoloured = vec![0u64; levels];
    // one record per live lake and level; half of seeds x levels covers a random field.  A guess that is too small
    // costs a second transform (WS_ERR_CAPACITY reports the exact count), never a wrong answer.
    let mut cap = (seeds.len().max(1) * levels / 2 + 1024).min(1 << 26);
    let mut lakes: Vec<hip_ffi::ws_lake>;
    let mut n = 0usize;
    loop {
        lakes = vec![hip_ffi::ws_lake::default(); cap];
        let rc = shim::with_ctx(|ctx| unsafe {
            let rc = hip_ffi::ws_transform_to_list(ctx, merging as c_int, std_img.as_ptr(), h, w, stride, packed.as_ptr(),
                                                   seeds.len(), &o, lakes.as_mut_ptr(), cap, &mut n, offsets.as_mut_ptr(),
                                                   uncoloured.as_mut_ptr());
            if rc != hip_ffi::WS_ERR_CAPACITY {
                shim::check(ctx, rc, "ws_transform_to_list");
            }
            rc
        });
        if rc == hip_ffi::WS_ERR_CAPACITY && n > cap {
            cap = n;
            continue;
        }
        break;
    }
    (0..levels)
        .map(|l| {
            let mut sizes = vec![0usize; ph * pw + 1];
            sizes[UNCOLOURED] = uncoloured[l] as usize;
            for rec in &lakes[offsets[l] as usize..offsets[l + 1] as usize] {
                sizes[rec.colour as usize] = rec.area as usize;
            }
            (l as u8, sizes)
        })
        .collect()
}

/// One slice's lists in sparse form: (level, uncoloured pixels, [(colour, area)]) per level.
pub type SparseLists = Vec<(u8, usize, Vec<(usize, usize)>)>;

/// transform_to_list of every slice of a cube, with each slice's own local minima as its seeds: one call of
/// `ws_transform_to_list_batch`.  Returns the slices' lists and their seed counts.
fn run_to_list_cube(merging: bool, opt: &Options, cube: nd::ArrayView3<u8>) -> (Vec<SparseLists>, Vec<usize>) {
    let (n, h, w) = cube.dim();
    let std_cube = cube.as_standard_layout();      // contiguous (slice, row, column); a copy only if the view is strided
    let o = opt.ffi();
    let levels = opt.max_water_level as usize + 1;
    let mut offsets = vec![0u64; n * levels + 1];
    let mut uncoloured = vec![0u64; n * levels];
    let mut n_seeds = vec![0usize; n];
    // one record per pixel of the cube (a random field needs ~10, a smooth map far fewer); a guess that is too small costs a
    // second transform (WS_ERR_CAPACITY reports the exact count), never a wrong answer
    let mut cap = (n * h * w + 1024).min(1 << 28);
    let mut lakes: Vec<hip_ffi::ws_lake>;
    let mut total = 0usize;
    let mut failed = 0usize;
    loop {
        lakes = vec![hip_ffi::ws_lake::default(); cap];
        let rc = shim::with_ctx(|ctx| unsafe {
            let rc = hip_ffi::ws_transform_to_list_batch(ctx, merging as c_int, std_cube.as_ptr(), n, h, w, w, h * w, std::ptr::null(),
                                                         std::ptr::null(), &o, lakes.as_mut_ptr(), cap, &mut total, offsets.as_mut_ptr(),
                                                         uncoloured.as_mut_ptr(), n_seeds.as_mut_ptr(), &mut failed);
            if rc != hip_ffi::WS_ERR_CAPACITY {
                shim::check(ctx, rc, "ws_transform_to_list_batch");
            }
            rc
        });
        if rc == hip_ffi::WS_ERR_CAPACITY && total > cap {
            cap = total;
            continue;
        }
        break;
    }
    let lists = (0..n)
        .map(|k| {
            (0..levels)
                .map(|l| {
                    let b = k * levels + l;
                    let recs = lakes[offsets[b] as usize..offsets[b + 1] as usize].iter().map(|r| (r.colour as usize, r.area as usize)).collect();
                    (l as u8, uncoloured[b] as usize, recs)
                })
                .collect()
        })
        .collect();
    (lists, n_seeds)
}

/// One slice's planes of transform_history for chosen water levels: (level, label plane) in the order of the levels.
pub type HistoryPlanes = Vec<(u8, nd::Array2<usize>)>;

/// transform_history of every slice of a cube for the water levels in `levels` (any order, repeats allowed, at most 256), with
/// each slice's own local minima as its seeds: one call of `ws_transform_history_batch`.  Returns the slices' planes and their
/// seed counts.
fn run_history_cube(merging: bool, opt: &Options, cube: nd::ArrayView3<u8>, levels: &[u8]) -> (Vec<HistoryPlanes>, Vec<usize>) {
    let (n, h, w) = cube.dim();
    let std_cube = cube.as_standard_layout();
    let o = opt.ffi();
    let (ph, pw) = opt.plane(h, w);
    let nl = levels.len();
    let mut planes = nd::Array4::<usize>::zeros((n, nl, ph, pw));
    let mut n_seeds = vec![0usize; n];
    let mut failed = 0usize;
    shim::with_ctx(|ctx| unsafe {
        let rc = hip_ffi::ws_transform_history_batch(ctx, merging as c_int, std_cube.as_ptr(), n, h, w, w, h * w, std::ptr::null(),
                                                     std::ptr::null(), &o, levels.as_ptr(), nl, planes.as_mut_ptr() as *mut u64,
                                                     n_seeds.as_mut_ptr(), &mut failed);
        shim::check(ctx, rc, "ws_transform_history_batch");
    });
    let out = (0..n)
        .map(|k| (0..nl).map(|j| (levels[j], planes.slice(nd::s![k, j, .., ..]).to_owned())).collect())
        .collect();
    (out, n_seeds)
}

fn history_hook(ctx: HookCtx) -> (u8, nd::Array2<usize>) {
    (ctx.water_level, ctx.colours.to_owned()) // lib.rs:1545, 1831
}

impl<T> Watershed<T> for SegmentingWatershed<T> {
    /// lib.rs:1810-1822 with the intended semantics: the labels after the last water level (`ws_segment`).
    fn transform(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)]) -> nd::Array2<usize> {
        let (h, w) = input.dim();
        let (std_img, stride) = shim::standard(&input);
        let packed = shim::pack_seeds(seeds);
        let o = self.opt.ffi();
        let mut out = nd::Array2::<usize>::zeros(self.opt.plane(h, w));
        shim::with_ctx(|ctx| unsafe {
            let rc = hip_ffi::ws_segment(ctx, std_img.as_ptr(), h, w, stride, packed.as_ptr(), seeds.len(), &o,
                                         out.as_mut_ptr() as *mut u64);
            shim::check(ctx, rc, "ws_segment");
        });
        out
    }
    /// lib.rs:1638-1808
    fn transform_with_hook(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)]) -> Vec<T> {
        run_with_hook(false, &self.opt, self.wlvl_hook, input, seeds, None)
    }
    /// lib.rs:1837-1847
    fn transform_to_list(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)]) -> Vec<(u8, Vec<usize>)> {
        run_to_list(false, &self.opt, input, seeds)
    }
    /// lib.rs:1824-1835
    fn transform_history(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)]) -> Vec<(u8, nd::Array2<usize>)> {
        run_with_hook(false, &self.opt, Some(history_hook as fn(HookCtx) -> _), input, seeds, None)
    }
}

impl<T> SegmentingWatershed<T> {
    /// Not in the reference: its README's call pair (lib.rs:73-86), `transform(input, &find_local_minima(input))`, as ONE
    /// call of the library (`ws_segment_minima`): the seeds never cross PCIe as (usize, usize) pairs unless asked for.
    /// Returns the labels and, with `want_seeds`, the seed list the labels are numbered by (colour i + 1 = entry i).
    pub fn transform_from_minima(&self, input: nd::ArrayView2<u8>, want_seeds: bool) -> (nd::Array2<usize>, Vec<(usize, usize)>) {
        let (h, w) = input.dim();
        let (std_img, stride) = shim::standard(&input);
        let o = self.opt.ffi();
        let mut out = nd::Array2::<usize>::zeros(self.opt.plane(h, w));
        // at most one strict maximum per 2 x 2 block of the interior
        let cap = if want_seeds && h >= 3 && w >= 3 { ((h - 1) / 2 + 1) * ((w - 1) / 2 + 1) } else { 0 };
        let mut packed = vec![0u64; 2 * cap];
        let mut n = 0usize;
        shim::with_ctx(|ctx| unsafe {
            let rc = hip_ffi::ws_segment_minima(ctx, std_img.as_ptr(), h, w, stride, &o, out.as_mut_ptr() as *mut u64,
                                                if cap != 0 { packed.as_mut_ptr() } else { std::ptr::null_mut() }, cap, &mut n);
            shim::check(ctx, rc, "ws_segment_minima");
        });
        let seeds = if want_seeds { packed.chunks_exact(2).take(n).map(|p| (p[0] as usize, p[1] as usize)).collect() } else { Vec::new() };
        (out, seeds)
    }

    /// Not in the reference: what its integration tests loop over (tests/integration.rs:267,356 -- `find_local_minima` +
    /// `transform` for one slice of a cube after the other) as ONE call of the library (`ws_segment_batch`): the slices take
    /// turns on internal contexts, so one slice's upload, another's transform and a third's label copy overlap.  Slice k of
    /// the result is exactly `transform(cube[k], &find_local_minima(cube[k]))`.
    pub fn transform_cube(&self, cube: nd::ArrayView3<u8>) -> nd::Array3<usize> {
        let (n, h, w) = cube.dim();
        let std_cube = cube.as_standard_layout();      // contiguous (slice, row, column); a copy only if the view is strided
        let o = self.opt.ffi();
        let (ph, pw) = self.opt.plane(h, w);
        let mut out = nd::Array3::<usize>::zeros((n, ph, pw));
        let mut failed = 0usize;
        shim::with_ctx(|ctx| unsafe {
            let rc = hip_ffi::ws_segment_batch(ctx, std_cube.as_ptr(), n, h, w, w, h * w, std::ptr::null(), std::ptr::null(), &o,
                                               out.as_mut_ptr() as *mut u64, std::ptr::null_mut(), &mut failed);
            shim::check(ctx, rc, "ws_segment_batch");
        });
        out
    }

    /// Not in the reference: `transform_to_list(cube[k], &find_local_minima(cube[k]))` for every slice of a cube, as one call
    /// (`ws_transform_to_list_batch`), in sparse form -- per slice and level the uncoloured count and the (colour, area) of every
    /// lake with pixels, in no particular order -- and the number of minima of every slice.
    pub fn transform_to_list_cube(&self, cube: nd::ArrayView3<u8>) -> (Vec<SparseLists>, Vec<usize>) {
        run_to_list_cube(false, &self.opt, cube)
    }

    /// Not in the reference: `transform_history` of every slice of a cube (seeds: each slice's `find_local_minima`) for the water
    /// levels in `levels` only, as one call (`ws_transform_history_batch`): per slice, (level, label plane) in the order of
    /// `levels` -- and the number of minima of every slice.
    pub fn transform_history_cube(&self, cube: nd::ArrayView3<u8>, levels: &[u8]) -> (Vec<HistoryPlanes>, Vec<usize>) {
        run_history_cube(false, &self.opt, cube, levels)
    }
}

impl<T> Watershed<T> for MergingWatershed<T> {
    /// lib.rs:1524-1536: a stub in the reference (zeros, interior 123, seeds ignored); kept for drop-in fidelity.
    fn transform(&self, input: nd::ArrayView2<u8>, _seeds: &[(usize, usize)]) -> nd::Array2<usize> {
        let (h, w) = input.dim();
        let mut out = nd::Array2::<usize>::zeros((h, w));
        let rc = unsafe { hip_ffi::ws_merge_transform_stub(h, w, out.as_mut_ptr() as *mut u64) };
        assert_eq!(rc, hip_ffi::WS_OK);
        out
    }
    /// lib.rs:1328-1522
    fn transform_with_hook(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)]) -> Vec<T> {
        run_with_hook(true, &self.opt, self.wlvl_hook, input, seeds, None)
    }
    /// lib.rs:1551-1561
    fn transform_to_list(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)]) -> Vec<(u8, Vec<usize>)> {
        run_to_list(true, &self.opt, input, seeds)
    }
    /// lib.rs:1538-1549
    fn transform_history(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)]) -> Vec<(u8, nd::Array2<usize>)> {
        run_with_hook(true, &self.opt, Some(history_hook as fn(HookCtx) -> _), input, seeds, None)
    }
}

/// The merging transform's lake hierarchy (`MergingWatershed::merge_tree`): `nodes[c]` is seed colour c's record.
pub struct MergeTree {
    pub nodes: Vec<hip_ffi::ws_tree_node>,
    pub labels: Option<nd::Array2<usize>>,
}

impl MergeTree {
    pub const ALIVE: u32 = hip_ffi::WS_TREE_ALIVE;
    /// colour -> canonical id of its lake after water level `level`: follow `parent` while `death_level <= level`.
    pub fn roots_at(&self, level: u32) -> Vec<u32> {
        (0..self.nodes.len() as u32)
            .map(|c| {
                let mut x = c;
                while self.nodes[x as usize].death_level <= level {
                    x = self.nodes[x as usize].parent;
                }
                x
            })
            .collect()
    }
    /// colour -> the first node of its parent chain that `cut` keeps: alive, or `area >= min_area` and `n_leaves >= min_leaves`.
    pub fn cut_table(&self, cut: &hip_ffi::ws_tree_cut) -> Vec<u32> {
        (0..self.nodes.len() as u32)
            .map(|c| {
                let mut x = c;
                loop {
                    let n = &self.nodes[x as usize];
                    if n.death_level == Self::ALIVE || (n.area >= cut.min_area && n.n_leaves >= cut.min_leaves) {
                        break x;
                    }
                    x = n.parent;
                }
            })
            .collect()
    }
    /// The same with catalogue thresholds (`ws_lake_cut`): `stats` is the catalogue of the tree's flood (`merge_tree_stats`); a
    /// node is also kept only if its `sum_w`, `w_max` and depth -- `death_level - w_min` where that is positive, else 0 -- reach
    /// the cut's.
    pub fn cut_table_stats(&self, cut: &hip_ffi::ws_lake_cut, stats: &[hip_ffi::ws_lake_stats]) -> Vec<u32> {
        assert_eq!(stats.len(), self.nodes.len(), "one catalogue record per tree record");
        (0..self.nodes.len() as u32)
            .map(|c| {
                let mut x = c;
                loop {
                    let (n, s) = (&self.nodes[x as usize], &stats[x as usize]);
                    let depth = if n.death_level != Self::ALIVE && n.death_level > s.w_min { n.death_level - s.w_min } else { 0 };
                    if n.death_level == Self::ALIVE
                        || (n.area >= cut.min_area && n.n_leaves >= cut.min_leaves && s.sum_w >= cut.min_sum_w && s.w_max >= cut.min_w_max
                            && depth >= cut.min_depth)
                    {
                        break x;
                    }
                    x = n.parent;
                }
            })
            .collect()
    }
}

/// What `MergingWatershed::tree_cut` returns: `planes[k]` shows every pixel the lake `cuts[k]` leaves it in (0: hidden);
/// `lakes[offsets[k] .. offsets[k + 1]]` are cut k's (colour, pixels) records in increasing colour, `hidden[k]` its pixels that show 0.
pub struct TreeCut {
    pub tree: MergeTree,
    pub planes: Vec<nd::Array2<usize>>,
    pub lakes: Vec<hip_ffi::ws_lake>,
    pub offsets: Vec<u64>,
    pub hidden: Vec<u64>,
}

/// What `MergingWatershed::tree_cut_stats` returns: a `TreeCut` and the lake catalogue of the same flood.
pub struct LakeCut {
    pub cut: TreeCut,
    pub stats: Vec<hip_ffi::ws_lake_stats>,
}

/// What `MergingWatershed::tree_cut_catalogue` returns: a `LakeCut`, `region_stats[i]` the record of the pixels `cut.lakes[i]`
/// counts -- the region of that colour in its cut, which is not the catalogue's record of the colour -- and `hidden_stats[k]` the
/// record of the pixels cut k shows as 0.
pub struct CutCatalogue {
    pub cut: LakeCut,
    pub region_stats: Vec<hip_ffi::ws_lake_stats>,
    pub hidden_stats: Vec<hip_ffi::ws_lake_stats>,
}

impl<T> MergingWatershed<T> {
    /// Not in the reference: `tree_cut_stats` with the regions the cuts show measured in the same call
    /// (`ws_merge_tree_cut_catalogue`): the source list of every cut.  `weights` as `tree_cut_stats`.
    pub fn tree_cut_catalogue(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)], weights: Option<nd::ArrayView2<u16>>,
                              cuts: &[hip_ffi::ws_lake_cut]) -> CutCatalogue {
        assert!(!cuts.is_empty() && cuts.len() <= 32, "tree_cut_catalogue takes 1 ..= 32 cuts");
        let (h, w) = input.dim();
        let (std_img, stride) = shim::standard(&input);
        let packed = shim::pack_seeds(seeds);
        let o = self.opt.ffi();
        let (ph, pw) = self.opt.plane(h, w);
        let k = cuts.len();
        let plane = weights.map(|a| {
            assert_eq!(a.dim(), (h, w), "weights must have the image's shape");
            a.as_standard_layout().into_owned()
        });
        let (wt_ptr, wt_dtype) = match plane.as_ref() {
            Some(a) => (a.as_ptr() as *const std::ffi::c_void, hip_ffi::WS_U16),
            None => (std::ptr::null(), 0),
        };
        let mut nodes = vec![hip_ffi::ws_tree_node::default(); seeds.len() + 1];
        let mut stats = vec![hip_ffi::ws_lake_stats::default(); seeds.len() + 1];
        let mut flat = vec![0u64; k * ph * pw];
        let cap = seeds.len().min(ph * pw).max(1) * k;      // a cut shows no more colours than there are, or pixels
        let mut lakes = vec![hip_ffi::ws_lake { colour: 0, area: 0 }; cap];
        let mut region_stats = vec![hip_ffi::ws_lake_stats::default(); cap];
        let mut hidden_stats = vec![hip_ffi::ws_lake_stats::default(); k];
        let (mut offsets, mut hidden, mut total) = (vec![0u64; k + 1], vec![0u64; k], 0usize);
        shim::with_ctx(|ctx| unsafe {
            let rc = hip_ffi::ws_merge_tree_cut_catalogue(ctx, std_img.as_ptr(), h, w, stride, packed.as_ptr(), seeds.len(), &o, wt_ptr, wt_dtype, w,
                                                          cuts.as_ptr(), k, nodes.as_mut_ptr(), stats.as_mut_ptr(), flat.as_mut_ptr(),
                                                          lakes.as_mut_ptr(), region_stats.as_mut_ptr(), cap, &mut total, offsets.as_mut_ptr(),
                                                          hidden.as_mut_ptr(), hidden_stats.as_mut_ptr());
            shim::check(ctx, rc, "ws_merge_tree_cut_catalogue");
        });
        lakes.truncate(total);
        region_stats.truncate(total);
        let planes = flat.chunks((ph * pw).max(1)).map(|p| nd::Array2::from_shape_vec((ph, pw), p.iter().map(|&v| v as usize).collect()).expect("plane shape")).collect();
        CutCatalogue { cut: LakeCut { cut: TreeCut { tree: MergeTree { nodes, labels: None }, planes, lakes, offsets, hidden }, stats }, region_stats,
                       hidden_stats }
    }

    /// Not in the reference: `tree_cut` with the lake catalogue of the same flood (`ws_merge_tree_stats_cut`): the cuts may also
    /// ask for a summed weight, a peak and a depth (`ws_lake_cut`).  `weights`: a u16 plane of the image's shape (`None`: the image
    /// itself weighs).
    pub fn tree_cut_stats(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)], weights: Option<nd::ArrayView2<u16>>,
                          cuts: &[hip_ffi::ws_lake_cut]) -> LakeCut {
        assert!(!cuts.is_empty() && cuts.len() <= 32, "tree_cut_stats takes 1 ..= 32 cuts");
        let (h, w) = input.dim();
        let (std_img, stride) = shim::standard(&input);
        let packed = shim::pack_seeds(seeds);
        let o = self.opt.ffi();
        let (ph, pw) = self.opt.plane(h, w);
        let k = cuts.len();
        let plane = weights.map(|a| {
            assert_eq!(a.dim(), (h, w), "weights must have the image's shape");
            a.as_standard_layout().into_owned()
        });
        let (wt_ptr, wt_dtype) = match plane.as_ref() {
            Some(a) => (a.as_ptr() as *const std::ffi::c_void, hip_ffi::WS_U16),
            None => (std::ptr::null(), 0),
        };
        let mut nodes = vec![hip_ffi::ws_tree_node::default(); seeds.len() + 1];
        let mut stats = vec![hip_ffi::ws_lake_stats::default(); seeds.len() + 1];
        let mut flat = vec![0u64; k * ph * pw];
        let cap = seeds.len().min(ph * pw).max(1) * k;      // a cut shows no more colours than there are, or pixels
        let mut lakes = vec![hip_ffi::ws_lake { colour: 0, area: 0 }; cap];
        let (mut offsets, mut hidden, mut total) = (vec![0u64; k + 1], vec![0u64; k], 0usize);
        shim::with_ctx(|ctx| unsafe {
            let rc = hip_ffi::ws_merge_tree_stats_cut(ctx, std_img.as_ptr(), h, w, stride, packed.as_ptr(), seeds.len(), &o, wt_ptr, wt_dtype, w,
                                                      cuts.as_ptr(), k, nodes.as_mut_ptr(), stats.as_mut_ptr(), flat.as_mut_ptr(),
                                                      lakes.as_mut_ptr(), cap, &mut total, offsets.as_mut_ptr(), hidden.as_mut_ptr());
            shim::check(ctx, rc, "ws_merge_tree_stats_cut");
        });
        lakes.truncate(total);
        let planes = flat.chunks((ph * pw).max(1)).map(|p| nd::Array2::from_shape_vec((ph, pw), p.iter().map(|&v| v as usize).collect()).expect("plane shape")).collect();
        LakeCut { cut: TreeCut { tree: MergeTree { nodes, labels: None }, planes, lakes, offsets, hidden }, stats }
    }

    /// Not in the reference: the label planes and lake lists of the merge tree pruned by `cuts` (1 ..= 32 of them), the whole
    /// route in one call (`ws_merge_tree_cut`).
    pub fn tree_cut(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)], cuts: &[hip_ffi::ws_tree_cut]) -> TreeCut {
        assert!(!cuts.is_empty() && cuts.len() <= 32, "tree_cut takes 1 ..= 32 cuts");
        let (h, w) = input.dim();
        let (std_img, stride) = shim::standard(&input);
        let packed = shim::pack_seeds(seeds);
        let o = self.opt.ffi();
        let (ph, pw) = self.opt.plane(h, w);
        let k = cuts.len();
        let mut nodes = vec![hip_ffi::ws_tree_node::default(); seeds.len() + 1];
        let mut flat = vec![0u64; k * ph * pw];
        let cap = seeds.len().min(ph * pw).max(1) * k;      // a cut shows no more colours than there are, or pixels
        let mut lakes = vec![hip_ffi::ws_lake { colour: 0, area: 0 }; cap];
        let (mut offsets, mut hidden, mut total) = (vec![0u64; k + 1], vec![0u64; k], 0usize);
        shim::with_ctx(|ctx| unsafe {
            let rc = hip_ffi::ws_merge_tree_cut(ctx, std_img.as_ptr(), h, w, stride, packed.as_ptr(), seeds.len(), &o, cuts.as_ptr(), k,
                                                nodes.as_mut_ptr(), flat.as_mut_ptr(), lakes.as_mut_ptr(), cap, &mut total,
                                                offsets.as_mut_ptr(), hidden.as_mut_ptr());
            shim::check(ctx, rc, "ws_merge_tree_cut");
        });
        lakes.truncate(total);
        let planes = flat.chunks((ph * pw).max(1)).map(|p| nd::Array2::from_shape_vec((ph, pw), p.iter().map(|&v| v as usize).collect()).expect("plane shape")).collect();
        TreeCut { tree: MergeTree { nodes, labels: None }, planes, lakes, offsets, hidden }
    }

    /// Not in the reference: the merging `transform_to_list(cube[k], &find_local_minima(cube[k]))` of every slice of a cube as one
    /// call; as `SegmentingWatershed::transform_to_list_cube`.
    pub fn transform_to_list_cube(&self, cube: nd::ArrayView3<u8>) -> (Vec<SparseLists>, Vec<usize>) {
        run_to_list_cube(true, &self.opt, cube)
    }
    /// Not in the reference: the merging `transform_history` of every slice of a cube for chosen water levels as one call (planes
    /// of canonical ids); as `SegmentingWatershed::transform_history_cube`.
    pub fn transform_history_cube(&self, cube: nd::ArrayView3<u8>, levels: &[u8]) -> (Vec<HistoryPlanes>, Vec<usize>) {
        run_history_cube(true, &self.opt, cube, levels)
    }
    /// Not in the reference: the lake hierarchy of the merging transform -- which lake swallowed which, after what water level,
    /// how big each was -- as one record per seed colour (index 0 ..= seeds.len()) from one flood; no plane is written
    /// (`ws_merge_tree`).  With `want_labels` also the segmenting label plane the colours refer to.
    pub fn merge_tree(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)], want_labels: bool) -> MergeTree {
        let (h, w) = input.dim();
        let (std_img, stride) = shim::standard(&input);
        let packed = shim::pack_seeds(seeds);
        let o = self.opt.ffi();
        let mut nodes = vec![hip_ffi::ws_tree_node::default(); seeds.len() + 1];
        let mut labels = if want_labels { Some(nd::Array2::<usize>::zeros(self.opt.plane(h, w))) } else { None };
        let lab_ptr = match labels.as_mut() {
            Some(a) => a.as_slice_mut().expect("standard layout").as_mut_ptr() as *mut u64,
            None => std::ptr::null_mut(),
        };
        shim::with_ctx(|ctx| unsafe {
            let rc = hip_ffi::ws_merge_tree(ctx, std_img.as_ptr(), h, w, stride, packed.as_ptr(), seeds.len(), &o, nodes.as_mut_ptr(), lab_ptr);
            shim::check(ctx, rc, "ws_merge_tree");
        });
        MergeTree { nodes, labels }
    }
    /// Not in the reference: `merge_tree` and a catalogue of its lakes from the same flood (`ws_merge_tree_stats`): record c of
    /// the second value holds the weighted and plain first moments, the box, the extrema and the first peak pixel of the pixels
    /// `nodes[c].area` counts, record 0 those of the pixels never coloured, in the coordinates of the padded plane.  `weights`:
    /// a u16 plane of the image's shape (`None`: the image itself weighs).
    pub fn merge_tree_stats(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)], weights: Option<nd::ArrayView2<u16>>,
                            want_labels: bool) -> (MergeTree, Vec<hip_ffi::ws_lake_stats>) {
        let (h, w) = input.dim();
        let (std_img, stride) = shim::standard(&input);
        let packed = shim::pack_seeds(seeds);
        let o = self.opt.ffi();
        let plane = weights.map(|a| {
            assert_eq!(a.dim(), (h, w), "weights must have the image's shape");
            a.as_standard_layout().into_owned()
        });
        let (wt_ptr, wt_dtype) = match plane.as_ref() {
            Some(a) => (a.as_ptr() as *const std::ffi::c_void, hip_ffi::WS_U16),
            None => (std::ptr::null(), 0),
        };
        let mut nodes = vec![hip_ffi::ws_tree_node::default(); seeds.len() + 1];
        let mut stats = vec![hip_ffi::ws_lake_stats::default(); seeds.len() + 1];
        let mut labels = if want_labels { Some(nd::Array2::<usize>::zeros(self.opt.plane(h, w))) } else { None };
        let lab_ptr = match labels.as_mut() {
            Some(a) => a.as_slice_mut().expect("standard layout").as_mut_ptr() as *mut u64,
            None => std::ptr::null_mut(),
        };
        shim::with_ctx(|ctx| unsafe {
            let rc = hip_ffi::ws_merge_tree_stats(ctx, std_img.as_ptr(), h, w, stride, packed.as_ptr(), seeds.len(), &o, wt_ptr, wt_dtype, w,
                                                  nodes.as_mut_ptr(), stats.as_mut_ptr(), lab_ptr);
            shim::check(ctx, rc, "ws_merge_tree_stats");
        });
        (MergeTree { nodes, labels }, stats)
    }
    /// Not in the reference: `merge_tree_stats` and the second moments of every lake from the same flood (`ws_merge_tree_shapes`):
    /// record c of the third value holds the exact 128-bit sums of v row^2, v col^2, v row col, row^2, col^2 and row col over the
    /// pixels `nodes[c].area` counts, each as (low, high) 64 bits, in the coordinates of the padded plane.  `weights` as
    /// `merge_tree_stats`.
    pub fn merge_tree_shapes(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)], weights: Option<nd::ArrayView2<u16>>,
                             want_labels: bool) -> (MergeTree, Vec<hip_ffi::ws_lake_stats>, Vec<hip_ffi::ws_lake_shape>) {
        let (h, w) = input.dim();
        let (std_img, stride) = shim::standard(&input);
        let packed = shim::pack_seeds(seeds);
        let o = self.opt.ffi();
        let plane = weights.map(|a| {
            assert_eq!(a.dim(), (h, w), "weights must have the image's shape");
            a.as_standard_layout().into_owned()
        });
        let (wt_ptr, wt_dtype) = match plane.as_ref() {
            Some(a) => (a.as_ptr() as *const std::ffi::c_void, hip_ffi::WS_U16),
            None => (std::ptr::null(), 0),
        };
        let mut nodes = vec![hip_ffi::ws_tree_node::default(); seeds.len() + 1];
        let mut stats = vec![hip_ffi::ws_lake_stats::default(); seeds.len() + 1];
        let mut shapes = vec![hip_ffi::ws_lake_shape::default(); seeds.len() + 1];
        let mut labels = if want_labels { Some(nd::Array2::<usize>::zeros(self.opt.plane(h, w))) } else { None };
        let lab_ptr = match labels.as_mut() {
            Some(a) => a.as_slice_mut().expect("standard layout").as_mut_ptr() as *mut u64,
            None => std::ptr::null_mut(),
        };
        shim::with_ctx(|ctx| unsafe {
            let rc = hip_ffi::ws_merge_tree_shapes(ctx, std_img.as_ptr(), h, w, stride, packed.as_ptr(), seeds.len(), &o, wt_ptr, wt_dtype, w,
                                                   nodes.as_mut_ptr(), stats.as_mut_ptr(), shapes.as_mut_ptr(), lab_ptr);
            shim::check(ctx, rc, "ws_merge_tree_shapes");
        });
        (MergeTree { nodes, labels }, stats, shapes)
    }
    /// Not in the reference: `merge_tree(cube[k], &find_local_minima(cube[k]), want_labels)` of every slice of a cube as one call
    /// (`ws_merge_tree_batch`: slices that stack share one flood, one set of per-level unions and one fold launch per level).
    /// Returns the trees, in the slices' own colours, and the number of minima of every slice.
    pub fn merge_tree_cube(&self, cube: nd::ArrayView3<u8>, want_labels: bool) -> (Vec<MergeTree>, Vec<usize>) {
        let (n, h, w) = cube.dim();
        let std_cube = cube.as_standard_layout();
        let o = self.opt.ffi();
        let (ph, pw) = self.opt.plane(h, w);
        // minima are rarely denser than one pixel in eight; a too small guess is answered with the count before any flood
        let mut cap = n * (h * w / 8 + 1);
        let mut flat = vec![hip_ffi::ws_tree_node::default(); cap];
        let mut labels = if want_labels { Some(nd::Array3::<usize>::zeros((n, ph, pw))) } else { None };
        let lab_ptr = match labels.as_mut() {
            Some(a) => a.as_slice_mut().expect("standard layout").as_mut_ptr() as *mut u64,
            None => std::ptr::null_mut(),
        };
        let mut n_seeds = vec![0usize; n];
        let (mut total, mut failed) = (0usize, 0usize);
        shim::with_ctx(|ctx| unsafe {
            for attempt in 0..2 {
                let rc = hip_ffi::ws_merge_tree_batch(ctx, std_cube.as_ptr(), n, h, w, w, h * w, std::ptr::null(), std::ptr::null(), &o,
                                                      flat.as_mut_ptr(), cap, &mut total, lab_ptr, n_seeds.as_mut_ptr(), &mut failed);
                if rc == hip_ffi::WS_ERR_CAPACITY && total > cap && attempt == 0 {
                    cap = total;
                    flat.resize(cap, hip_ffi::ws_tree_node::default());
                    continue;
                }
                shim::check(ctx, rc, "ws_merge_tree_batch");
                break;
            }
        });
        let mut at = 0usize;
        let trees = (0..n)
            .map(|k| {
                let nodes = flat[at..at + n_seeds[k] + 1].to_vec();
                at += n_seeds[k] + 1;
                MergeTree { nodes, labels: labels.as_ref().map(|a| a.slice(nd::s![k, .., ..]).to_owned()) }
            })
            .collect();
        (trees, n_seeds)
    }
    /// Not in the reference: `merge_tree_stats(cube[k], &find_local_minima(cube[k]), weights[k], want_labels)` of every slice of a
    /// cube as one call (`ws_merge_tree_stats_batch`: slices that stack share one flood, one set of per-level unions and one fold
    /// launch per level of the tree and of the statistics).  Returns per slice the tree and its records, in the slice's own
    /// colours, rows, columns and peak pixels, and the number of minima of every slice.  `weights`: a u16 cube of the cube's
    /// shape (`None`: the cube itself weighs).
    pub fn merge_tree_stats_cube(&self, cube: nd::ArrayView3<u8>, weights: Option<nd::ArrayView3<u16>>,
                                 want_labels: bool) -> (Vec<(MergeTree, Vec<hip_ffi::ws_lake_stats>)>, Vec<usize>) {
        let (n, h, w) = cube.dim();
        let std_cube = cube.as_standard_layout();
        let o = self.opt.ffi();
        let (ph, pw) = self.opt.plane(h, w);
        let planes = weights.map(|a| {
            assert_eq!(a.dim(), (n, h, w), "weights must have the cube's shape");
            a.as_standard_layout().into_owned()
        });
        let (wt_ptr, wt_dtype) = match planes.as_ref() {
            Some(a) => (a.as_ptr() as *const std::ffi::c_void, hip_ffi::WS_U16),
            None => (std::ptr::null(), 0),
        };
        // (as merge_tree_cube: a too small guess is answered with the count before any flood)
        let mut cap = n * (h * w / 8 + 1);
        let mut flat = vec![hip_ffi::ws_tree_node::default(); cap];
        let mut records = vec![hip_ffi::ws_lake_stats::default(); cap];
        let mut labels = if want_labels { Some(nd::Array3::<usize>::zeros((n, ph, pw))) } else { None };
        let lab_ptr = match labels.as_mut() {
            Some(a) => a.as_slice_mut().expect("standard layout").as_mut_ptr() as *mut u64,
            None => std::ptr::null_mut(),
        };
        let mut n_seeds = vec![0usize; n];
        let (mut total, mut failed) = (0usize, 0usize);
        shim::with_ctx(|ctx| unsafe {
            for attempt in 0..2 {
                let rc = hip_ffi::ws_merge_tree_stats_batch(ctx, std_cube.as_ptr(), n, h, w, w, h * w, std::ptr::null(), std::ptr::null(), &o,
                                                            wt_ptr, wt_dtype, w, h * w, flat.as_mut_ptr(), records.as_mut_ptr(), cap, &mut total,
                                                            lab_ptr, n_seeds.as_mut_ptr(), &mut failed);
                if rc == hip_ffi::WS_ERR_CAPACITY && total > cap && attempt == 0 {
                    cap = total;
                    flat.resize(cap, hip_ffi::ws_tree_node::default());
                    records.resize(cap, hip_ffi::ws_lake_stats::default());
                    continue;
                }
                shim::check(ctx, rc, "ws_merge_tree_stats_batch");
                break;
            }
        });
        let mut at = 0usize;
        let out = (0..n)
            .map(|k| {
                let nodes = flat[at..at + n_seeds[k] + 1].to_vec();
                let stats = records[at..at + n_seeds[k] + 1].to_vec();
                at += n_seeds[k] + 1;
                (MergeTree { nodes, labels: labels.as_ref().map(|a| a.slice(nd::s![k, .., ..]).to_owned()) }, stats)
            })
            .collect();
        (out, n_seeds)
    }
    /// Not in the reference: `merge_tree_shapes(cube[k], &find_local_minima(cube[k]), weights[k], want_labels)` of every slice of a
    /// cube as one call (`ws_merge_tree_shapes_batch`: slices that stack run the shape kernels once over the stack, after the
    /// tree's and the statistics').  Returns per slice the tree, its first-moment records and its second moments, in the slice's
    /// own colours, rows and columns, and the number of minima of every slice.  `weights` as `merge_tree_stats_cube`.
    #[allow(clippy::type_complexity)]
    pub fn merge_tree_shapes_cube(&self, cube: nd::ArrayView3<u8>, weights: Option<nd::ArrayView3<u16>>, want_labels: bool)
                                  -> (Vec<(MergeTree, Vec<hip_ffi::ws_lake_stats>, Vec<hip_ffi::ws_lake_shape>)>, Vec<usize>) {
        let (n, h, w) = cube.dim();
        let std_cube = cube.as_standard_layout();
        let o = self.opt.ffi();
        let (ph, pw) = self.opt.plane(h, w);
        let planes = weights.map(|a| {
            assert_eq!(a.dim(), (n, h, w), "weights must have the cube's shape");
            a.as_standard_layout().into_owned()
        });
        let (wt_ptr, wt_dtype) = match planes.as_ref() {
            Some(a) => (a.as_ptr() as *const std::ffi::c_void, hip_ffi::WS_U16),
            None => (std::ptr::null(), 0),
        };
        // (as merge_tree_cube: a too small guess is answered with the count before any flood)
        let mut cap = n * (h * w / 8 + 1);
        let mut flat = vec![hip_ffi::ws_tree_node::default(); cap];
        let mut records = vec![hip_ffi::ws_lake_stats::default(); cap];
        let mut moments = vec![hip_ffi::ws_lake_shape::default(); cap];
        let mut labels = if want_labels { Some(nd::Array3::<usize>::zeros((n, ph, pw))) } else { None };
        let lab_ptr = match labels.as_mut() {
            Some(a) => a.as_slice_mut().expect("standard layout").as_mut_ptr() as *mut u64,
            None => std::ptr::null_mut(),
        };
        let mut n_seeds = vec![0usize; n];
        let (mut total, mut failed) = (0usize, 0usize);
        shim::with_ctx(|ctx| unsafe {
            for attempt in 0..2 {
                let rc = hip_ffi::ws_merge_tree_shapes_batch(ctx, std_cube.as_ptr(), n, h, w, w, h * w, std::ptr::null(), std::ptr::null(), &o,
                                                             wt_ptr, wt_dtype, w, h * w, flat.as_mut_ptr(), records.as_mut_ptr(),
                                                             moments.as_mut_ptr(), cap, &mut total, lab_ptr, n_seeds.as_mut_ptr(), &mut failed);
                if rc == hip_ffi::WS_ERR_CAPACITY && total > cap && attempt == 0 {
                    cap = total;
                    flat.resize(cap, hip_ffi::ws_tree_node::default());
                    records.resize(cap, hip_ffi::ws_lake_stats::default());
                    moments.resize(cap, hip_ffi::ws_lake_shape::default());
                    continue;
                }
                shim::check(ctx, rc, "ws_merge_tree_shapes_batch");
                break;
            }
        });
        let mut at = 0usize;
        let out = (0..n)
            .map(|k| {
                let rows = at..at + n_seeds[k] + 1;
                at += n_seeds[k] + 1;
                (MergeTree { nodes: flat[rows.clone()].to_vec(), labels: labels.as_ref().map(|a| a.slice(nd::s![k, .., ..]).to_owned()) },
                 records[rows.clone()].to_vec(), moments[rows].to_vec())
            })
            .collect();
        (out, n_seeds)
    }
    /// Not in the reference: `tree_cut_catalogue(cube[k], &find_local_minima(cube[k]), weights[k], cuts)` of every slice of a cube
    /// as one call (`ws_merge_tree_cut_catalogue_batch`: slices that stack share one flood, and every stacked group is cut once,
    /// while its stamps are on the device).  Returns per slice the `CutCatalogue` of the slice alone -- its own colours, rows,
    /// columns and peak pixels, offsets from 0 -- and the number of minima of every slice.  `weights` as `merge_tree_stats_cube`.
    pub fn merge_tree_cut_catalogue_cube(&self, cube: nd::ArrayView3<u8>, weights: Option<nd::ArrayView3<u16>>,
                                         cuts: &[hip_ffi::ws_lake_cut]) -> (Vec<CutCatalogue>, Vec<usize>) {
        assert!(!cuts.is_empty() && cuts.len() <= 32, "merge_tree_cut_catalogue_cube takes 1 ..= 32 cuts");
        let (n, h, w) = cube.dim();
        let std_cube = cube.as_standard_layout();
        let o = self.opt.ffi();
        let (ph, pw) = self.opt.plane(h, w);
        let k = cuts.len();
        let planes_w = weights.map(|a| {
            assert_eq!(a.dim(), (n, h, w), "weights must have the cube's shape");
            a.as_standard_layout().into_owned()
        });
        let (wt_ptr, wt_dtype) = match planes_w.as_ref() {
            Some(a) => (a.as_ptr() as *const std::ffi::c_void, hip_ffi::WS_U16),
            None => (std::ptr::null(), 0),
        };
        // (as merge_tree_cube: a too small guess of the records is answered with the count before any flood; of the lists, with the need)
        let mut rec_cap = n * (h * w / 8 + 1);
        let mut cap = rec_cap.min(n * ph * pw).max(1) * k;
        let mut flat = vec![hip_ffi::ws_tree_node::default(); rec_cap];
        let mut records = vec![hip_ffi::ws_lake_stats::default(); rec_cap];
        let mut lakes = vec![hip_ffi::ws_lake { colour: 0, area: 0 }; cap];
        let mut region = vec![hip_ffi::ws_lake_stats::default(); cap];
        let mut hidden_stats = vec![hip_ffi::ws_lake_stats::default(); n * k];
        let mut planes = vec![0u64; n * k * ph * pw];
        let (mut offsets, mut hidden) = (vec![0u64; n * k + 1], vec![0u64; n * k]);
        let mut n_seeds = vec![0usize; n];
        let (mut total, mut got, mut failed) = (0usize, 0usize, 0usize);
        shim::with_ctx(|ctx| unsafe {
            for attempt in 0..3 {
                let rc = hip_ffi::ws_merge_tree_cut_catalogue_batch(ctx, std_cube.as_ptr(), n, h, w, w, h * w, std::ptr::null(), std::ptr::null(), &o,
                                                                    wt_ptr, wt_dtype, w, h * w, cuts.as_ptr(), k, flat.as_mut_ptr(),
                                                                    records.as_mut_ptr(), rec_cap, &mut total, planes.as_mut_ptr(),
                                                                    lakes.as_mut_ptr(), region.as_mut_ptr(), cap, &mut got, offsets.as_mut_ptr(),
                                                                    hidden.as_mut_ptr(), hidden_stats.as_mut_ptr(), n_seeds.as_mut_ptr(), &mut failed);
                if rc == hip_ffi::WS_ERR_CAPACITY && total > rec_cap && attempt < 2 {
                    rec_cap = total;
                    flat.resize(rec_cap, hip_ffi::ws_tree_node::default());
                    records.resize(rec_cap, hip_ffi::ws_lake_stats::default());
                    continue;
                }
                if rc == hip_ffi::WS_ERR_CAPACITY && got > cap && attempt < 2 {
                    cap = got;
                    lakes.resize(cap, hip_ffi::ws_lake { colour: 0, area: 0 });
                    region.resize(cap, hip_ffi::ws_lake_stats::default());
                    continue;
                }
                shim::check(ctx, rc, "ws_merge_tree_cut_catalogue_batch");
                break;
            }
        });
        let npx = ph * pw;
        let mut at = 0usize;
        let out = (0..n)
            .map(|s| {
                let nodes = flat[at..at + n_seeds[s] + 1].to_vec();
                let stats = records[at..at + n_seeds[s] + 1].to_vec();
                at += n_seeds[s] + 1;
                let (lo, hi) = (offsets[s * k] as usize, offsets[(s + 1) * k] as usize);
                let slice_planes = (0..k)
                    .map(|j| {
                        let p = &planes[(s * k + j) * npx..(s * k + j + 1) * npx];
                        nd::Array2::from_shape_vec((ph, pw), p.iter().map(|&v| v as usize).collect()).expect("plane shape")
                    })
                    .collect();
                let cut = TreeCut { tree: MergeTree { nodes, labels: None }, planes: slice_planes, lakes: lakes[lo..hi].to_vec(),
                                    offsets: offsets[s * k..(s + 1) * k + 1].iter().map(|&x| x - lo as u64).collect(),
                                    hidden: hidden[s * k..(s + 1) * k].to_vec() };
                CutCatalogue { cut: LakeCut { cut, stats }, region_stats: region[lo..hi].to_vec(), hidden_stats: hidden_stats[s * k..(s + 1) * k].to_vec() }
            })
            .collect();
        (out, n_seeds)
    }
    /// Not in the reference: the merged label plane after the last level (canonical ids: the smallest seed colour of
    /// every lake).  The reference's own `transform` is the stub above.
    pub fn transform_final(&self, input: nd::ArrayView2<u8>, seeds: &[(usize, usize)]) -> nd::Array2<usize> {
        let (h, w) = input.dim();
        let mut out = nd::Array2::<usize>::zeros(self.opt.plane(h, w));
        run_with_hook::<()>(true, &self.opt, None, input, seeds, Some(&mut out));
        out
    }
}

#[cfg(test)]
mod tests {
    // needs an MI355X and libws_hip.so: `WS_HIP_LIB_DIR=.. cargo test`; mirrors README.md:55-70 of the reference
    use super::prelude::*;
    use ndarray as nd;
    use ndarray_rand::{rand_distr::Uniform, RandomExt};

    #[test]
    fn quickstart() {
        let rf = nd::Array2::<u8>::random((512, 512), Uniform::new(0, 254));
        let watershed = TransformBuilder::default().build_segmenting().unwrap();
        let mins = watershed.find_local_minima(rf.view());
        let output = watershed.transform(rf.view(), &mins);
        assert_eq!(output.dim(), (512, 512));
        for (i, &(r, c)) in mins.iter().enumerate() {
            assert_eq!(output[(r, c)], i + 1);
        }
        let lists = TransformBuilder::default().build_merging().unwrap().transform_to_list(rf.view(), &mins);
        assert_eq!(lists.len(), 255);
        assert!(lists.iter().all(|(_, v)| v.len() == 512 * 512 + 1 && v.iter().sum::<usize>() == 512 * 512));
    }

    #[test]
    fn builder_errors() {
        assert!(matches!(TransformBuilder::default().set_max_water_lvl(255).build_segmenting(), Err(crate::BuildErr::MaxToHigh(255))));
        assert!(matches!(TransformBuilder::default().set_max_water_lvl(0).build_merging(), Err(crate::BuildErr::MaxToLow(0))));
    }
}
