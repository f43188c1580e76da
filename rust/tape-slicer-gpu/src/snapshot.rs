//! The compute of lib/snapshot over libtapeec's snapshot codec (te_snapshot_*): `encode_chunks`
//! is what `encode_snapshot` (lib/snapshot/src/encode.rs:62-154) does between lz4 and its track
//! records, `assemble` what the reader's fan-in plus `outer_decode_segments` and the prefix
//! stripping of `decode_snapshot_log` do (network/protocol/src/snapshot.rs:159-172,
//! lib/snapshot/src/decode.rs:90-150).  Both keep the reference's shapes: encode_snapshot builds
//! its `SnapshotChunk`s from the tuples, and the reader hands its verified slices over instead of
//! decoding track by track.
use crate::{decode_status, detail, encode_status, fatal, ClayCoder};
use tapeec_sys as ffi;

pub const GROUP_SIZE: usize = 20;
pub type Hash = [u8; 32];

/// SnapshotError's variants that come out of the engine (lib/snapshot/src/lib.rs).
#[derive(Clone, Debug, PartialEq, Eq)]
pub enum SnapshotError {
    NoGroups,
    NoChunks,
    MissingChunk { chunk: usize },
    InsufficientGroups { chunk: u64, got: usize, need: usize },
    ChunkPayload(String),
    OuterEncode(String),
    OuterDecode(String),
    ClayDecode(String),
}

/// One chunk of `encode_chunks`, in track_number order (chunk * total_groups + group).
pub struct EncodedChunk {
    pub group: u64,
    pub chunk: u64,
    pub leaves: [Hash; GROUP_SIZE],
    pub root: Hash,
    pub slices: [Vec<u8>; GROUP_SIZE],
    /// BlobEncoding::size and stripe_count: from the symbol length (encode.rs:136-146)
    pub size: u64,
    pub stripe_size: u64,
    pub stripe_count: u64,
}

fn plan(coder: &ClayCoder, len: usize, total_groups: usize)
    -> Result<(ffi::te_snapshot_plan_info, Vec<ffi::te_snapshot_segment>), SnapshotError> {
    let mut info: ffi::te_snapshot_plan_info = unsafe { std::mem::zeroed() };
    let r = unsafe { ffi::te_snapshot_plan(coder.raw.as_ptr(), len as u64, total_groups as u32, &mut info, std::ptr::null_mut(), 0) };
    match r {
        0 => {}
        20 => return Err(SnapshotError::NoGroups),
        s => return Err(SnapshotError::OuterEncode(format!("status {s}: {}", detail()))),
    }
    let mut segs: Vec<ffi::te_snapshot_segment> = vec![unsafe { std::mem::zeroed() }; info.segments as usize];
    let r = unsafe { ffi::te_snapshot_plan(coder.raw.as_ptr(), len as u64, total_groups as u32, &mut info, segs.as_mut_ptr(), segs.len()) };
    if r != 0 { fatal(r) }
    Ok((info, segs))
}

/// encode_snapshot's segment cut, outer RS, headers, Clay encode and commitments for the
/// lz4-compressed log, in one device pipeline (te_snapshot_encode_host).
pub fn encode_chunks(coder: &mut ClayCoder, compressed: &[u8], total_groups: usize)
    -> Result<Vec<(u64, u64, [Hash; GROUP_SIZE], Hash, [Vec<u8>; GROUP_SIZE])>, SnapshotError> {
    Ok(encode_chunks_full(coder, compressed, total_groups)?.into_iter().map(|c| (c.group, c.chunk, c.leaves, c.root, c.slices)).collect())
}

pub fn encode_chunks_full(coder: &mut ClayCoder, compressed: &[u8], total_groups: usize) -> Result<Vec<EncodedChunk>, SnapshotError> {
    let (info, segs) = plan(coder, compressed.len(), total_groups)?;
    let nch = info.chunks as usize;
    let mut slices = vec![0u8; info.total_slice_bytes as usize];
    let mut leaves = vec![0u8; nch * GROUP_SIZE * 32];
    let mut roots = vec![0u8; nch * 32];
    let r = unsafe {
        ffi::te_snapshot_encode_host(coder.raw.as_ptr(), compressed.as_ptr(), compressed.len() as u64, total_groups as u32,
                                     slices.as_mut_ptr(), slices.len(), leaves.as_mut_ptr(), roots.as_mut_ptr())
    };
    encode_status(r).map_err(|e| SnapshotError::OuterEncode(format!("{e:?}")))?;
    let mut out = Vec::with_capacity(nch);
    for (s, g) in segs.iter().enumerate() {
        let sl = g.geom.slice_len as usize;
        for group in 0..total_groups {
            let t = s * total_groups + group;
            let base = g.slices_off as usize + group * GROUP_SIZE * sl;
            let mut lv = [[0u8; 32]; GROUP_SIZE];
            for (i, h) in lv.iter_mut().enumerate() { h.copy_from_slice(&leaves[(t * GROUP_SIZE + i) * 32..][..32]); }
            let mut root = [0u8; 32];
            root.copy_from_slice(&roots[t * 32..][..32]);
            out.push(EncodedChunk {
                group: group as u64, chunk: s as u64, leaves: lv, root,
                slices: core::array::from_fn(|i| slices[base + i * sl..][..sl].to_vec()),
                size: g.size, stripe_size: g.geom.stripe_size, stripe_count: g.stripe_count,
            });
        }
    }
    Ok(out)
}

/// One fetched chunk track: its group, its verified `(leaf_index, slice)` pairs (at least 7) and,
/// for the engine to check them again on the device, optionally its BlobEncoding::leaves.
pub struct FetchedTrack<'a> {
    pub group: u64,
    pub slices: Vec<(usize, &'a [u8])>,
    pub leaves: Option<&'a [Hash; GROUP_SIZE]>,
}

/// Clay-decode every track, file each symbol under its header's segment, outer-decode every
/// segment, strip the length prefixes and concatenate: the compressed log, ready for lz4.
/// Tracks that do not decode are skipped, as the reader skips them.
pub fn assemble(coder: &mut ClayCoder, tracks: &[FetchedTrack<'_>], total_groups: usize) -> Result<Vec<u8>, SnapshotError> {
    if total_groups == 0 { return Err(SnapshotError::NoGroups); }
    let verified = !tracks.is_empty() && tracks.iter().all(|t| t.leaves.is_some());
    let mut descs: Vec<ffi::te_snapshot_track> = Vec::with_capacity(tracks.len());
    let (mut blob, mut metas, mut leaves) = (Vec::<u8>::new(), Vec::<u8>::new(), Vec::<u8>::new());
    for t in tracks {
        let sl = t.slices.first().map(|(_, d)| d.len()).unwrap_or(0);
        let off = blob.len();
        blob.resize(off + (GROUP_SIZE * sl + 63) / 64 * 64, 0);
        let mut mask = 0u32;
        for (i, d) in &t.slices {
            if *i >= GROUP_SIZE || d.len() != sl { return Err(SnapshotError::ClayDecode("InvalidLayout".into())); }
            blob[off + i * sl..][..sl].copy_from_slice(d);
            mask |= 1 << i;
        }
        let mut meta = [0u8; 48];
        if sl >= 48 { meta.copy_from_slice(&t.slices[0].1[sl - 48..]); }
        metas.extend_from_slice(&meta);
        if let Some(l) = t.leaves { for h in l { leaves.extend_from_slice(h); } }
        descs.push(ffi::te_snapshot_track {
            group: t.group as u32, pad_: 0,
            obj: ffi::te_decode_object { slices_off: off as u64, slice_len: sl as u64, avail_mask: mask, pad_: 0, out_off: 0 },
        });
    }
    let cap = blob.len();
    let mut out = vec![0u8; cap.max(1)];
    let mut status = vec![0i32; tracks.len().max(1)];
    let mut segment = vec![0u64; tracks.len().max(1)];
    let mut out_len = 0u64;
    let r = unsafe {
        ffi::te_snapshot_decode_host(coder.raw.as_ptr(), total_groups as u32, blob.as_ptr(), descs.as_ptr(), metas.as_ptr(),
                                     if verified { leaves.as_ptr() } else { std::ptr::null() }, tracks.len(), out.as_mut_ptr(),
                                     cap as u64, &mut out_len, status.as_mut_ptr(), std::ptr::null_mut(), segment.as_mut_ptr())
    };
    if r == 3 {
        let d = detail();
        let nums: Vec<u64> = d.split(|c: char| !c.is_ascii_digit()).filter_map(|t| t.parse().ok()).collect();
        return Err(if d.starts_with("MissingChunk") {
            SnapshotError::MissingChunk { chunk: *nums.first().unwrap_or(&0) as usize }
        } else if d.starts_with("InsufficientGroups") {
            SnapshotError::InsufficientGroups { got: *nums.first().unwrap_or(&0) as usize, need: *nums.get(1).unwrap_or(&0) as usize,
                                                chunk: *nums.get(2).unwrap_or(&0) }
        } else if d.starts_with("NoChunks") {
            SnapshotError::NoChunks
        } else {
            SnapshotError::OuterDecode("NotEnoughSlices".into())
        });
    }
    if r == 5 { return Err(SnapshotError::ChunkPayload(detail())); }
    decode_status(r).map_err(|e| SnapshotError::OuterDecode(format!("{e:?}")))?;
    out.truncate(out_len as usize);
    Ok(out)
}

/// te_snapshot_launch_stats of the coder's last snapshot call.
pub fn launch_stats(coder: &ClayCoder) -> ffi::te_snapshot_stats {
    let mut st: ffi::te_snapshot_stats = unsafe { std::mem::zeroed() };
    let r = unsafe { ffi::te_snapshot_launch_stats(coder.raw.as_ptr(), &mut st) };
    if r != 0 { fatal(r) }
    st
}
