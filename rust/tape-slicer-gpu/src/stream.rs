//! The stream writer's ordered encode stage (sdk/src/stream/write.rs:332-362: up to
//! min(cores, 4) chunk encodes in flight, handed on in order through FuturesOrdered) over
//! te_stream_writer: one GPU pipeline per ClayCoder (one per device), windows enqueued without
//! blocking, completed in submission order.  Each window is `encode_with_proofs` of its objects
//! (sdk/src/codec/encoder.rs:220-260).  `StreamReader` is its read counterpart over te_stream_reader.
use crate::{decode_status, encode_status, pack_objects, slicer_cfg, ClayCoder, DecodeError, EncodeError, ErasureCoder, PinnedBuf,
            PinnedPool};
use std::collections::BTreeMap;
use tapeec_sys as ffi;

struct Pending { data: PinnedBuf, objs: Vec<ffi::te_object>, out: crate::EncodedWindow }

/// Who hashes the leaves (te_stream_writer_set_hashing): `Auto` picks per window -- the SDK's
/// 64 MiB chunks (9.7 MB slices, <= 4 in flight) hash on the library's host pool as their slices
/// land, batches of small objects on the device.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Hashing { Auto, Device, Host }

pub struct StreamWriter<'a> {
    raw: *mut ffi::te_stream_writer,
    coders: Vec<&'a mut ClayCoder>,  // the handles outlive the writer (borrowed)
    pending: BTreeMap<u64, Pending>,
    pool: PinnedPool,                 // pinned input / slice buffers, reused across windows
}

impl<'a> StreamWriter<'a> {
    /// group_bytes: hashing group per handle (0 = 8 GiB); height: SLICE_TREE_HEIGHT.
    pub fn new(coders: Vec<&'a mut ClayCoder>, group_bytes: usize) -> Self {
        let raws: Vec<*mut ffi::te_clay> = coders.iter().map(|c| c.raw.as_ptr()).collect();
        let cfg = slicer_cfg(&*coders[0], true, 0);
        let mut w = std::ptr::null_mut();
        let r = unsafe {
            ffi::te_stream_writer_new(raws.as_ptr(), raws.len(), &cfg, ffi::TE_SLICE_TREE_HEIGHT as u32, group_bytes, &mut w)
        };
        if r != 0 { crate::fatal(r) }
        Self { raw: w, coders, pending: BTreeMap::new(), pool: PinnedPool::default() }
    }

    pub fn set_hashing(&mut self, h: Hashing) {
        let mode = match h { Hashing::Auto => ffi::TE_HASH_AUTO, Hashing::Device => ffi::TE_HASH_DEVICE, Hashing::Host => ffi::TE_HASH_HOST };
        let r = unsafe { ffi::te_stream_writer_set_hashing(self.raw, mode as i32) };
        if r != 0 { crate::fatal(r) }
    }

    /// Hand a completed window's pinned slice buffer back for reuse (after the slices are stored).
    pub fn recycle(&mut self, w: crate::EncodedWindow) { self.pool.give(w.slices) }

    /// Enqueue one window; returns its ticket.  The window's buffers stay owned here (stable
    /// addresses for the asynchronous copies) until `next` hands them back.
    pub fn submit(&mut self, objects: &[&[u8]], chunk_index: &[u64]) -> Result<u64, EncodeError> {
        let (data, objs, out_len) = pack_objects(&*self.coders[0], &mut self.pool, objects, chunk_index);
        let n = self.coders[0].n();
        let h = ffi::TE_SLICE_TREE_HEIGHT as usize;
        let mut p = Pending { data, objs, out: crate::EncodedWindow {
            slices: self.pool.take(out_len as usize), leaf_hashes: vec![0; objects.len() * n * 32],
            roots: vec![0; objects.len() * 32], proofs: vec![0; objects.len() * n * h * 32] } };
        let mut t = 0u64;
        let r = unsafe {
            ffi::te_stream_submit(self.raw, p.data.as_ptr(), p.objs.as_ptr(), p.objs.len(), p.out.slices.as_mut_ptr(),
                                  p.out.leaf_hashes.as_mut_ptr(), p.out.roots.as_mut_ptr(), p.out.proofs.as_mut_ptr(), &mut t)
        };
        // a failed window keeps its ticket: `next` reports it in order (its buffers are no longer
        // referenced by the device once submit has returned)
        if t != 0 { self.pending.insert(t, p); }
        encode_status(r)?;
        Ok(t)
    }

    /// Windows submitted and not yet handed back by `next`.
    pub fn in_flight(&self) -> usize { self.pending.len() }

    /// The oldest window, completed (FuturesOrdered::next).
    pub fn next(&mut self) -> Option<Result<crate::EncodedWindow, EncodeError>> {
        let (&t, _) = self.pending.iter().next()?;
        let r = unsafe { ffi::te_stream_wait(self.raw, t) };
        let p = self.pending.remove(&t)?;
        self.pool.give(p.data);  // the window's input buffer is free once it has completed
        Some(encode_status(r).map(|_| p.out))
    }
}

impl Drop for StreamWriter<'_> {
    fn drop(&mut self) { unsafe { ffi::te_stream_writer_free(self.raw) } }
}

/// One decoded window of the stream reader: the objects' bytes back to back in one pinned buffer.
/// Track i is `bytes[offsets[i]..offsets[i] + lens[i]]` if `status[i]` is Ok; `hash_mismatches[i]`
/// is the mask of fetched slices that failed `verify_slice` (decode.rs:121-139).
pub struct DecodedWindow {
    pub bytes: PinnedBuf,
    pub offsets: Vec<usize>,
    pub lens: Vec<usize>,
    pub status: Vec<Result<(), DecodeError>>,
    pub hash_mismatches: Vec<u32>,
}

struct PendingRead { slices: PinnedBuf, out: DecodedWindow, raw_status: Vec<i32> }

/// The read counterpart of `StreamWriter` over te_stream_reader: the tracks of a multi-track
/// object (the gateway's decode_track_bytes, one call per track, decode.rs:28-91; the SDK's
/// read_track) as windows that are enqueued without blocking and completed in submission order,
/// so one window's upload, the kernels of the one before and the download of the one before that
/// overlap.
pub struct StreamReader<'a> {
    raw: *mut ffi::te_stream_reader,
    coders: Vec<&'a mut ClayCoder>,  // the handles outlive the reader (borrowed)
    pending: BTreeMap<u64, PendingRead>,
    pool: PinnedPool,
}

impl<'a> StreamReader<'a> {
    pub fn new(coders: Vec<&'a mut ClayCoder>) -> Self {
        let raws: Vec<*mut ffi::te_clay> = coders.iter().map(|c| c.raw.as_ptr()).collect();
        let cfg = slicer_cfg(&*coders[0], true, 0);
        let mut r = std::ptr::null_mut();
        let s = unsafe { ffi::te_stream_reader_new(raws.as_ptr(), raws.len(), &cfg, &mut r) };
        if s != 0 { crate::fatal(s) }
        Self { raw: r, coders, pending: BTreeMap::new(), pool: PinnedPool::default() }
    }

    /// Hand a completed window's pinned buffer back for reuse (after the bytes are consumed).
    pub fn recycle(&mut self, w: DecodedWindow) { self.pool.give(w.bytes) }

    /// Enqueue one window: `tracks[i]` are the (slice index, slice bytes) a reader fetched for
    /// track i, `leaves[i]` its BlobEncoding::leaves (n hashes) for a verified read, or None for
    /// every track to decode without the check.  Returns the window's ticket.
    pub fn submit(&mut self, tracks: &[&[(usize, &[u8])]], leaves: Option<&[&[[u8; 32]]]>) -> Result<u64, DecodeError> {
        let n = self.coders[0].n();
        let mut objs = Vec::with_capacity(tracks.len());
        let mut metas = Vec::with_capacity(tracks.len() * ffi::TE_META_SIZE as usize);
        let (mut in_len, mut out_len) = (0usize, 0usize);
        let (mut offsets, mut lens) = (Vec::new(), Vec::new());
        for t in tracks {
            let first = t.first().ok_or(DecodeError::NotEnoughSlices)?.1;
            let slice_len = first.len();
            if slice_len < ffi::TE_META_SIZE as usize || t.iter().any(|(i, s)| *i >= n || s.len() != slice_len) {
                return Err(DecodeError::InvalidLayout);
            }
            let mut m = std::mem::MaybeUninit::<ffi::te_slice_metadata>::zeroed();
            decode_status(unsafe { ffi::te_slice_metadata_from_slice(first.as_ptr(), slice_len, m.as_mut_ptr()) })?;
            let blob_len = unsafe { m.assume_init() }.blob_len as usize;
            let mask = t.iter().fold(0u32, |a, (i, _)| a | 1u32 << i);
            objs.push(ffi::te_decode_object { slices_off: in_len as u64, slice_len: slice_len as u64, avail_mask: mask,
                                              pad_: 0, out_off: out_len as u64 });
            metas.extend_from_slice(&first[slice_len - ffi::TE_META_SIZE as usize..]);
            offsets.push(out_len);
            lens.push(blob_len);
            in_len += n * slice_len;
            out_len += blob_len;
        }
        // each slice at its slot i * slice_len of the track's range; absent slots are never read
        let mut slices = self.pool.take(in_len);
        for (t, o) in tracks.iter().zip(&objs) {
            for (i, s) in t.iter() {
                let at = o.slices_off as usize + i * s.len();
                slices[at..at + s.len()].copy_from_slice(s);
            }
        }
        let flat: Option<Vec<u8>> = leaves.map(|l| l.iter().flat_map(|t| t.iter().flatten().copied()).collect());
        if let Some(f) = &flat {
            if f.len() != tracks.len() * n * 32 { return Err(DecodeError::InvalidLayout); }
        }
        let mut p = PendingRead { slices, raw_status: vec![0; tracks.len()], out: DecodedWindow {
            bytes: self.pool.take(out_len), offsets, lens, status: Vec::new(), hash_mismatches: vec![0; tracks.len()] } };
        let mut t = 0u64;
        let r = unsafe {
            ffi::te_stream_read_submit(self.raw, p.slices.as_ptr(), objs.as_ptr(), metas.as_ptr(),
                                       flat.as_ref().map_or(std::ptr::null(), |f| f.as_ptr()), objs.len(),
                                       p.out.bytes.as_mut_ptr(), p.out.hash_mismatches.as_mut_ptr(),
                                       p.raw_status.as_mut_ptr(), &mut t)
        };
        // the library copies objs, metas and leaves; the pinned buffers and the per-track vectors
        // (heap storage: moving `p` does not move them) stay owned here until `next`
        if t == 0 {
            self.pool.give(p.slices);
            self.pool.give(p.out.bytes);
            decode_status(r)?;
            crate::fatal(r)
        }
        self.pending.insert(t, p);
        Ok(t)
    }

    /// Windows submitted and not yet handed back by `next`.
    pub fn in_flight(&self) -> usize { self.pending.len() }

    /// The oldest window, completed: per track Ok or `NotEnoughSlices` ("insufficient verified
    /// slices", decode.rs:160-170).  An engine failure of the window panics as elsewhere.
    pub fn next(&mut self) -> Option<DecodedWindow> {
        let (&t, _) = self.pending.iter().next()?;
        let r = unsafe { ffi::te_stream_read_wait(self.raw, t) };
        if r != 0 { crate::fatal(r) }
        let mut p = self.pending.remove(&t)?;
        self.pool.give(p.slices);
        p.out.status = p.raw_status.iter().map(|&s| decode_status(s)).collect();
        Some(p.out)
    }
}

impl Drop for StreamReader<'_> {
    fn drop(&mut self) { unsafe { ffi::te_stream_reader_free(self.raw) } }
}
