// binius_amd/host/transcript.hpp -- the seam between the mirrors and the caller's Fiat-Shamir transcript.
//
// A mirror hands every message to a TranscriptSource at the moment the reference writes it (TranscriptWriter::write_scalar_slice /
// write, crates/core/src/transcript/mod.rs:372-416) and asks it for every sample at the moment the reference draws it (CanSample::sample,
// CanSampleBits::sample_bits).  Two sources:
//
//   ArrayTranscript   the samples drawn before the call, as the array entry points of include/binius_amd_host.h take them: one
//                     array ("stream") per role, sample(stream, index) reads streams[stream][index]; what is written is dropped
//   LiveTranscript    the caller's bnh_transcript table: sample() draws the next value whatever stream and index say, write()
//                     hands the bytes on; a callback that returns non-zero is Error::Callback (BN_ERR_CALLBACK)
//
// The (stream, index) pair names a sample for the array form only.  A mirror that runs over a TranscriptSource therefore has ONE
// body for both forms, and it is causally clean exactly when its calls happen in the reference's order.
#pragma once
#include <array>
#include <string>
#include <utility>
#include <vector>

#include "../../include/binius_amd_host.h"
#include "compute_layer.hpp"

namespace binius_amd {

class TranscriptSource {
public:
	virtual ~TranscriptSource() = default;
	virtual B128 sample(int stream, size_t index) = 0;
	// n consecutive samples of one stream: transcript.sample_vec(n)
	virtual std::vector<B128> sample_vec(int stream, size_t first, size_t n)
	{
		std::vector<B128> v(n);
		for (size_t i = 0; i < n; i++) v[i] = sample(stream, first + i);
		return v;
	}
	// n x transcript.sample_bits(bits); the array form reads bit_samples[first .. first + n)
	virtual std::vector<uint64_t> sample_bits_vec(uint32_t bits, size_t first, size_t n) = 0;
	virtual void write(uint32_t channel, const void *bytes, size_t len) = 0;
	// Is this a caller's transcript, which reads what is written and must stay in step with the verifier's?  A mirror may skip work
	// that only serves write(), and draws that nothing uses, when it is not (the array form).
	virtual bool observes_writes() const { return true; }

	// scalars as 16-byte little-endian canonical-tower elements (the layout of B128 and bn_f128), digests as their 32 bytes
	void write_scalars(const B128 *v, size_t n, uint32_t channel = BNH_TR_MESSAGE)
	{
		if (n) write(channel, v, n * sizeof(B128));
	}
	void write_scalars(const std::vector<B128> &v, uint32_t channel = BNH_TR_MESSAGE) { write_scalars(v.data(), v.size(), channel); }
	void write_digest(const std::array<uint8_t, 32> &d, uint32_t channel = BNH_TR_MESSAGE) { write(channel, d.data(), d.size()); }
};

class ArrayTranscript : public TranscriptSource {
public:
	using Stream = std::pair<const B128 *, size_t>;
	explicit ArrayTranscript(std::vector<Stream> streams, const uint64_t *bit_samples = nullptr, size_t n_bit_samples = 0)
	    : streams_(std::move(streams)), bits_(bit_samples), n_bits_(n_bit_samples)
	{
	}
	static Stream stream(const std::vector<B128> &v) { return Stream{v.data(), v.size()}; }
	B128 sample(int stream, size_t index) override
	{
		if (stream < 0 || (size_t)stream >= streams_.size() || index >= streams_[(size_t)stream].second)
			throw Error(Error::InputValidation, "too few transcript samples (stream " + std::to_string(stream) + ", index " + std::to_string(index) + ")");
		return streams_[(size_t)stream].first[index];
	}
	std::vector<uint64_t> sample_bits_vec(uint32_t, size_t first, size_t n) override
	{
		if (first + n > n_bits_) throw Error(Error::InputValidation, "too few sampled indices");
		return std::vector<uint64_t>(bits_ + first, bits_ + first + n);
	}
	void write(uint32_t, const void *, size_t) override {}
	bool observes_writes() const override { return false; }

private:
	std::vector<Stream> streams_;
	const uint64_t *bits_;
	size_t n_bits_;
};

class LiveTranscript : public TranscriptSource {
public:
	// need_bits: the entry point draws sample_bits.  A null table or a null member it needs is InputValidation.
	explicit LiveTranscript(const bnh_transcript *table, bool need_bits = false) : t_(table)
	{
		if (!table || !table->write || !table->sample || (need_bits && !table->sample_bits))
			throw Error(Error::InputValidation, "null transcript table, or a null callback the entry point needs");
	}
	B128 sample(int, size_t) override
	{
		bn_f128 v{0, 0};
		if (t_->sample(t_->user, &v, 1) != 0) throw Error(Error::Callback, "the transcript's sample callback failed");
		return from_raw(v);
	}
	std::vector<B128> sample_vec(int, size_t, size_t n) override
	{
		static_assert(sizeof(B128) == sizeof(bn_f128), "a field element is one bn_f128");
		std::vector<B128> v(n);
		if (n && t_->sample(t_->user, reinterpret_cast<bn_f128 *>(v.data()), (uint32_t)n) != 0) throw Error(Error::Callback, "the transcript's sample callback failed");
		return v;
	}
	std::vector<uint64_t> sample_bits_vec(uint32_t bits, size_t, size_t n) override
	{
		std::vector<uint64_t> v(n);
		if (n && (!t_->sample_bits || t_->sample_bits(t_->user, bits, (uint32_t)n, v.data()) != 0)) throw Error(Error::Callback, "the transcript's sample_bits callback failed");
		return v;
	}
	void write(uint32_t channel, const void *bytes, size_t len) override
	{
		if (len && t_->write(t_->user, channel, bytes, len) != 0) throw Error(Error::Callback, "the transcript's write callback failed");
	}

private:
	const bnh_transcript *t_;
};

} // namespace binius_amd
