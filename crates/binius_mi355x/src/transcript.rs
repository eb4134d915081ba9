//! `ProverTranscript<Challenger>` behind the `bnh_transcript` table of `libbinius_amd_host.so` (include/binius_amd_host.h,
//! "Against a live transcript"): the adapter a prover hands to the `bnh_*_live` entry points, so that the compiled provers write
//! every message where the reference writes it and draw every sample where the reference draws it.
//!
//! `write` forwards the bytes as they come -- they are already in transcript byte order (`write_scalar_slice` of B128 is sixteen
//! little-endian bytes of the canonical-tower element; a digest is its 32 bytes) -- to `transcript.message()` or
//! `transcript.decommitment()`; `sample` is `CanSample::<B128>::sample`, `sample_bits` is `CanSampleBits::sample_bits`.
//! A panic inside a callback is caught and becomes a non-zero return (the entry point then returns `BN_ERR_CALLBACK`): nothing
//! unwinds through the C++ frames.  The callbacks run on the calling thread, inside the entry point; the adapter borrows the
//! transcript mutably for as long as the table is alive.
//!
//! Feature `provers` (pulls in `binius_core` for the transcript).

use std::{
	marker::PhantomData,
	os::raw::{c_int, c_void},
	panic::{catch_unwind, AssertUnwindSafe},
	slice,
};

use binius_core::{
	fiat_shamir::{CanSample, CanSampleBits, Challenger},
	transcript::ProverTranscript,
};
use binius_field::BinaryField128b as B128;

use crate::{
	ffi::{bn_f128, bnh_transcript, BNH_TR_DECOMMITMENT, BNH_TR_MESSAGE},
	to_ffi,
};

/// The table over a borrowed transcript.  `as_ptr()` is what a `bnh_*_live` entry point takes.
pub struct LiveTranscript<'a, C: Challenger> {
	table: bnh_transcript,
	_transcript: PhantomData<&'a mut ProverTranscript<C>>,
}

impl<'a, C: Challenger> LiveTranscript<'a, C> {
	pub fn new(transcript: &'a mut ProverTranscript<C>) -> Self {
		Self {
			table: bnh_transcript {
				user: (transcript as *mut ProverTranscript<C>).cast::<c_void>(),
				write: Some(write::<C>),
				sample: Some(sample::<C>),
				sample_bits: Some(sample_bits::<C>),
			},
			_transcript: PhantomData,
		}
	}

	pub fn as_ptr(&self) -> *const bnh_transcript {
		&self.table
	}
}

fn guarded(body: impl FnOnce()) -> c_int {
	match catch_unwind(AssertUnwindSafe(body)) {
		Ok(()) => 0,
		Err(_) => 1,
	}
}

unsafe extern "C" fn write<C: Challenger>(user: *mut c_void, channel: u32, bytes: *const c_void, len: u64) -> c_int {
	if user.is_null() || (bytes.is_null() && len != 0) || (channel != BNH_TR_MESSAGE && channel != BNH_TR_DECOMMITMENT) {
		return 1;
	}
	guarded(|| {
		let transcript = unsafe { &mut *user.cast::<ProverTranscript<C>>() };
		let data = if len == 0 { &[][..] } else { unsafe { slice::from_raw_parts(bytes.cast::<u8>(), len as usize) } };
		if channel == BNH_TR_MESSAGE {
			transcript.message().write_bytes(data);
		} else {
			transcript.decommitment().write_bytes(data);
		}
	})
}

unsafe extern "C" fn sample<C: Challenger>(user: *mut c_void, out: *mut bn_f128, n: u32) -> c_int {
	if user.is_null() || (out.is_null() && n != 0) {
		return 1;
	}
	guarded(|| {
		let transcript = unsafe { &mut *user.cast::<ProverTranscript<C>>() };
		for i in 0..n as usize {
			let value: B128 = transcript.sample();
			unsafe { out.add(i).write(to_ffi(value)) };
		}
	})
}

unsafe extern "C" fn sample_bits<C: Challenger>(user: *mut c_void, bits: u32, n: u32, out: *mut u64) -> c_int {
	if user.is_null() || (out.is_null() && n != 0) || bits > 32 {
		return 1; // (CanSampleBits<u32>: the reference draws at most 32 bits at a time)
	}
	guarded(|| {
		let transcript = unsafe { &mut *user.cast::<ProverTranscript<C>>() };
		for i in 0..n as usize {
			let value: u32 = transcript.sample_bits(bits as usize);
			unsafe { out.add(i).write(u64::from(value)) };
		}
	})
}
