//! The node's rebuild loop over the host rebuild pipeline: `repair::run`'s batches of
//! `repair_batch` tracks (network/node/src/features/spool/repair.rs:94-226) and their escalation
//! (recover.rs:77-244, `reconstruct` recover.rs:411-442), both ending in `verify_slice`
//! (repair.rs:340, recover.rs:216).  One call per batch instead of one `Slicer::repair` /
//! `reconstruct` plus a host hash per track; INTEGRATION.md shows the loop bound to these.
use crate::slicer_hook::{ObjectCfg, RepairPlan};
use crate::{decode_status, fatal, repair_status, ClayCoder, DecodeError, ErasureCoder, PinnedBuf, RepairError};
use tapeec_sys as ffi;

/// One track of a repair batch: its plan, where each named helper's fragment (the peer's
/// `extract_repair_data` reply) lies in the batch's helper buffer, where the repaired slice goes
/// in the output buffer, and the 48-byte metadata suffix.
pub struct RepairObject<'a> {
    pub plan: &'a RepairPlan,
    /// (helper slice, offset of its fragment in `helpers`); helpers the plan does not name are ignored
    pub fragments: Vec<(usize, u64)>,
    pub out_off: u64,
    pub metadata: [u8; 48],
}

/// One track of a recover batch: n slots of `slice_len` bytes at `slices_off` (only the slots in
/// `avail_mask` are read), the slice to rebuild and where it goes.
#[derive(Clone, Copy, Debug)]
pub struct RecoverObject { pub slices_off: u64, pub slice_len: u64, pub avail_mask: u32, pub lost: u32, pub out_off: u64 }

/// Per object of a verified recover: TE_OK or TE_ERR_NOT_ENOUGH_SLICES (nothing written), the
/// peers that failed their leaf, and whether the rebuilt slice verified.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct RecoverOutcome { pub status: i32, pub rejected_mask: u32, pub verified: bool }

/// te_repair_batch_host: every track of the batch repaired into `out`.  With `leaves` (n * 32
/// bytes per track) returns per track whether hash_leaf(repaired) == leaves[plan.lost]
/// (repair.rs:340); a track that fails escalates to `recover_batch`.  Without, every entry is true.
pub fn repair_batch(coder: &mut ClayCoder, helpers: &PinnedBuf, objects: &[RepairObject<'_>], leaves: Option<&[u8]>,
                    out: &mut PinnedBuf, window_bytes: usize) -> Result<Vec<bool>, RepairError> {
    let n = coder.n();
    if let Some(l) = leaves { assert_eq!(l.len(), objects.len() * n * 32, "leaves: n * 32 bytes per track") }
    let mut objs = Vec::with_capacity(objects.len());
    for o in objects {
        let mut d = ffi::te_repair_object { plan: o.plan.raw(), helper_off: [u64::MAX; ffi::TE_GROUP_SIZE as usize],
                                            out_off: o.out_off, metadata: o.metadata };
        for (h, off) in &o.fragments {
            if *h >= n { return Err(RepairError::InvalidSlice) }
            let len = unsafe { ffi::te_extract_repair_data_size(o.plan.raw(), *h as u32) } as u64;
            assert!(off + len <= helpers.len() as u64, "fragment past the helper buffer");
            d.helper_off[*h] = *off;
        }
        let len = o.plan.num_stripes as u64 * o.plan.chunk_size + ffi::TE_META_SIZE as u64;
        assert!(o.out_off + len <= out.capacity() as u64, "repaired slice past the output buffer");
        objs.push(d);
    }
    let mut ok = vec![1u32; objects.len()];
    let r = unsafe {
        ffi::te_repair_batch_host(coder.raw.as_ptr(), helpers.as_ptr(), objs.as_ptr(),
                                  leaves.map_or(std::ptr::null(), |l| l.as_ptr()), objs.len(), out.as_mut_ptr(),
                                  if leaves.is_some() { ok.as_mut_ptr() } else { std::ptr::null_mut() }, window_bytes)
    };
    repair_status(r, None)?;
    Ok(ok.into_iter().map(|v| v != 0).collect())
}

/// te_recover_batch_host: `reconstruct` for every track of the batch.  `metas`: one 48-byte suffix
/// per track.  With `leaves` the peers are verified first and the rebuilt slice after
/// (recover.rs:207-218); without, every outcome is (TE_OK, 0, true) and fewer than k present slices
/// is the call's error.
pub fn recover_batch(coder: &mut ClayCoder, cfg: &ObjectCfg, slices: &PinnedBuf, objects: &[RecoverObject],
                     metas: &[u8], leaves: Option<&[u8]>, out: &mut PinnedBuf, window_bytes: usize)
        -> Result<Vec<RecoverOutcome>, DecodeError> {
    let n = coder.n();
    assert_eq!(metas.len(), objects.len() * ffi::TE_META_SIZE as usize, "metas: 48 bytes per track");
    if let Some(l) = leaves { assert_eq!(l.len(), objects.len() * n * 32, "leaves: n * 32 bytes per track") }
    let mut objs = Vec::with_capacity(objects.len());
    for o in objects {
        let top = (32 - (o.avail_mask & ((1u64 << n) - 1) as u32).leading_zeros()) as u64;  // slots read
        assert!(o.slices_off + top * o.slice_len <= slices.len() as u64, "peer slice past the slice buffer");
        assert!(o.out_off + o.slice_len <= out.capacity() as u64, "rebuilt slice past the output buffer");
        objs.push(ffi::te_recover_object { slices_off: o.slices_off, slice_len: o.slice_len, avail_mask: o.avail_mask,
                                           lost: o.lost, out_off: o.out_off });
    }
    let c = cfg.ffi();
    let (mut rej, mut ok, mut st) = (vec![0u32; objects.len()], vec![1u32; objects.len()], vec![0i32; objects.len()]);
    let v = leaves.is_some();
    let r = unsafe {
        ffi::te_recover_batch_host(coder.raw.as_ptr(), &c, slices.as_ptr(), objs.as_ptr(), metas.as_ptr(),
                                   leaves.map_or(std::ptr::null(), |l| l.as_ptr()), objs.len(), out.as_mut_ptr(),
                                   if v { rej.as_mut_ptr() } else { std::ptr::null_mut() },
                                   if v { ok.as_mut_ptr() } else { std::ptr::null_mut() },
                                   if v { st.as_mut_ptr() } else { std::ptr::null_mut() }, window_bytes)
    };
    decode_status(r)?;
    Ok((0..objects.len()).map(|i| RecoverOutcome { status: st[i], rejected_mask: rej[i], verified: ok[i] != 0 }).collect())
}

/// te_slicer_recover_multi: `reconstruct` (recover.rs:411-442) for several lost slices of one
/// object.  A node that owns L spools of a group rebuilds them from one fetch of k peer slices: the
/// slices go to the device once, one decode rebuilds every slice index in `lost`.  Returns
/// (slice index, slice) in ascending index order.  A lost index whose slice is present, or none, is
/// the call's error.
pub fn recover_many(coder: &mut ClayCoder, cfg: &ObjectCfg, slices: &[(usize, &[u8])], lost: &[usize])
        -> Result<Vec<(usize, Vec<u8>)>, DecodeError> {
    let n = coder.n();
    if slices.is_empty() { return Err(DecodeError::NotEnoughSlices) }
    let slen = slices[0].1.len();
    let mut ptrs = vec![std::ptr::null::<u8>(); n];
    for (i, s) in slices {
        if *i >= n || s.len() != slen || !ptrs[*i].is_null() { return Err(DecodeError::InvalidLayout) }
        ptrs[*i] = s.as_ptr();
    }
    let mut want: Vec<usize> = lost.to_vec();
    want.sort_unstable();
    want.dedup();
    assert!(!want.is_empty() && want.len() == lost.len() && want.iter().all(|&i| i < n), "lost: distinct slice indices below n");
    let mask = want.iter().fold(0u32, |m, &i| m | 1u32 << i);
    let mut outs: Vec<Vec<u8>> = want.iter().map(|_| vec![0u8; slen]).collect();
    let optrs: Vec<*mut u8> = outs.iter_mut().map(|o| o.as_mut_ptr()).collect();
    let c = cfg.ffi();
    decode_status(unsafe {
        ffi::te_slicer_recover_multi(coder.raw.as_ptr(), &c, ptrs.as_ptr(), slen, mask, optrs.as_ptr())
    })?;
    Ok(want.into_iter().zip(outs).collect())
}

/// The last `recover_many` call on this coder: launches of the multi-output kernel, the most
/// passes a stripe took, its jobs and output rows, and the objects sent to each path.
pub fn recover_many_launch_stats(coder: &ClayCoder) -> ffi::te_recover_multi_stats {
    let mut st = ffi::te_recover_multi_stats { multi_launches: 0, passes: 0, jobs: 0, out_rows: 0, stripes: 0,
                                               split_stripes: 0, single_objects: 0, generic_objects: 0, multi_objects: 0 };
    let s = unsafe { ffi::te_clay_recover_multi_launch_stats(coder.raw.as_ptr(), &mut st) };
    if s != 0 { fatal(s) }
    st
}

/// The last `repair_batch` / `recover_batch` call on this coder: windows, objects, fragments or
/// slices and bytes uploaded, bytes copied back, where the leaves were hashed, host waits.
pub fn rebuild_launch_stats(coder: &ClayCoder) -> ffi::te_rebuild_launch_stats {
    let mut st = ffi::te_rebuild_launch_stats { windows: 0, objects: 0, pieces_uploaded: 0, bytes_h2d: 0, bytes_d2h: 0,
                                                slices_hashed_host: 0, slices_hashed_device: 0, host_waits: 0 };
    let s = unsafe { ffi::te_clay_rebuild_launch_stats(coder.raw.as_ptr(), &mut st) };
    if s != 0 { fatal(s) }
    st
}

/// The windows `repair_batch` would cut (te_repair_window_plan; host only).
pub fn repair_window_count(coder: &ClayCoder, objects: &[RepairObject<'_>], window_bytes: usize) -> usize {
    let objs: Vec<ffi::te_repair_object> = objects.iter().map(|o| ffi::te_repair_object {
        plan: o.plan.raw(), helper_off: [0; ffi::TE_GROUP_SIZE as usize], out_off: o.out_off, metadata: o.metadata }).collect();
    let mut nw = 0usize;
    let s = unsafe {
        ffi::te_repair_window_plan(coder.raw.as_ptr(), objs.as_ptr(), objs.len(), window_bytes, std::ptr::null_mut(), 0, &mut nw)
    };
    if s != 0 { fatal(s) }
    nw
}

/// The windows `recover_batch` would cut (te_recover_window_plan; host only).
pub fn recover_window_count(coder: &ClayCoder, objects: &[RecoverObject], window_bytes: usize) -> usize {
    let objs: Vec<ffi::te_recover_object> = objects.iter().map(|o| ffi::te_recover_object {
        slices_off: o.slices_off, slice_len: o.slice_len, avail_mask: o.avail_mask, lost: o.lost, out_off: o.out_off }).collect();
    let mut nw = 0usize;
    let s = unsafe {
        ffi::te_recover_window_plan(coder.raw.as_ptr(), objs.as_ptr(), objs.len(), window_bytes, std::ptr::null_mut(), 0, &mut nw)
    };
    if s != 0 { fatal(s) }
    nw
}
