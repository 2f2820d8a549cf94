/*
 * stream_host.cpp — agx_stream_* and agx_event_* of the C ABI (include/agx.h): streams (plain and masked to a set of compute units) and the
 * events that order them.  They know nothing of the engine.
 */
#include "agx_internal.hpp"

#include <chrono>
#include <mutex>
#include <thread>
#include <vector>

extern "C" {

int agx_stream_create(void **out)
{
	AGX_REQUIRE(out != nullptr, AGX_ERR_INVALID, "agx_stream_create: null argument");
	hipStream_t s = nullptr;
	AGX_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
	*out = s;
	return AGX_OK;
}
/* a stream whose kernels run only on the compute units whose bits are set in `mask` (bit i of word i / 32 = CU i): slices of a pool
 * that own disjoint parts of the chip */
namespace
{
	/* hipStreamDestroy of a CU-masked stream hangs on ROCm 7.2, so such a stream lives until the process exits — and therefore must not be
	 * created twice: the streams are cached process-wide by (device, mask).  A generator thread that sets its slices up again for every
	 * training iteration (GeneratorManager::generate, once per iteration in the reference) gets the same streams back instead of leaking a
	 * hardware queue per slice and iteration. */
	struct MaskedStream
	{
			int device, instance;
			std::vector<uint32_t> mask;
			hipStream_t stream;
	};
	std::mutex g_masked_streams_mutex;
	std::vector<MaskedStream> g_masked_streams;
}
int agx_stream_create_with_cu_mask(void **out, const uint32_t *mask, int words)
{
	return agx_stream_create_with_cu_mask_instance(out, mask, words, 0);
}
int agx_stream_create_with_cu_mask_instance(void **out, const uint32_t *mask, int words, int instance)
{
	AGX_REQUIRE(out != nullptr && mask != nullptr && words > 0, AGX_ERR_INVALID, "agx_stream_create_with_cu_mask: invalid argument");
	bool any = false;
	for (int i = 0; i < words; i++)
		any = any || mask[i] != 0u;
	AGX_REQUIRE(any, AGX_ERR_INVALID, "agx_stream_create_with_cu_mask: the mask selects no compute unit");
	int device = 0;
	AGX_HIP_CHECK(hipGetDevice(&device));
	std::vector<uint32_t> key(mask, mask + words);
	while (key.size() > 1 && key.back() == 0u)
		key.pop_back(); // (trailing zero words select nothing: the same mask)
	std::lock_guard<std::mutex> lock(g_masked_streams_mutex);
	for (const MaskedStream &m : g_masked_streams)
		if (m.device == device && m.instance == instance && m.mask == key)
		{
			*out = m.stream;
			return AGX_OK;
		}
	hipStream_t s = nullptr;
	AGX_HIP_CHECK(hipExtStreamCreateWithCUMask(&s, static_cast<uint32_t>(words), mask));
	g_masked_streams.push_back(MaskedStream { device, instance, key, s });
	*out = s;
	return AGX_OK;
}
int agx_stream_masked_count(void)
{
	std::lock_guard<std::mutex> lock(g_masked_streams_mutex);
	return static_cast<int>(g_masked_streams.size());
}
int agx_stream_destroy(void *stream)
{
	if (stream == nullptr)
		return AGX_OK;
	hipStream_t s = static_cast<hipStream_t>(stream);
	bool masked = false;
	{
		std::lock_guard<std::mutex> lock(g_masked_streams_mutex);
		for (const MaskedStream &m : g_masked_streams)
			masked = masked || (m.stream == s);
	}
	if (masked)
	{ // drained (outside the lock), not destroyed: it stays in the cache for the next caller
		AGX_HIP_CHECK(hipStreamSynchronize(s));
		return AGX_OK;
	}
	AGX_HIP_CHECK(hipStreamDestroy(s));
	return AGX_OK;
}
/* events: ordering between streams without the host (a slice's tower launch on the network partition waits for its search launch on the
 * search partition and the other way round) */
int agx_event_create(void **out)
{
	AGX_REQUIRE(out != nullptr, AGX_ERR_INVALID, "agx_event_create: null argument");
	hipEvent_t ev = nullptr;
	AGX_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
	*out = ev;
	return AGX_OK;
}
int agx_event_create_blocking(void **out)
{ // for agx_event_synchronize: the waiting host thread sleeps (hipEventBlockingSync) instead of spinning
	AGX_REQUIRE(out != nullptr, AGX_ERR_INVALID, "agx_event_create_blocking: null argument");
	hipEvent_t ev = nullptr;
	AGX_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventBlockingSync | hipEventDisableTiming));
	*out = ev;
	return AGX_OK;
}
int agx_event_synchronize(void *event)
{ // a SLEEPING wait: hipEventSynchronize spins in user space on this runtime even for a hipEventBlockingSync event (measured: the waiting
  // thread stays at 100 %), so the event is polled between 100 us naps — the callers wait for work that was queued steps ago
	AGX_REQUIRE(event != nullptr, AGX_ERR_INVALID, "agx_event_synchronize: null event");
	while (true)
	{
		const hipError_t st = hipEventQuery(static_cast<hipEvent_t>(event));
		if (st == hipSuccess)
			return AGX_OK;
		if (st != hipErrorNotReady)
			AGX_HIP_CHECK(st);
		std::this_thread::sleep_for(std::chrono::microseconds(100));
	}
}
int agx_event_record(void *event, void *stream)
{
	AGX_REQUIRE(event != nullptr, AGX_ERR_INVALID, "agx_event_record: null event");
	AGX_HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(event), static_cast<hipStream_t>(stream)));
	return AGX_OK;
}
int agx_stream_wait_event(void *stream, void *event)
{
	AGX_REQUIRE(event != nullptr, AGX_ERR_INVALID, "agx_stream_wait_event: null event");
	AGX_HIP_CHECK(hipStreamWaitEvent(static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(event), 0));
	return AGX_OK;
}
int agx_event_destroy(void *event)
{
	if (event != nullptr)
		AGX_HIP_CHECK(hipEventDestroy(static_cast<hipEvent_t>(event)));
	return AGX_OK;
}
int agx_stream_synchronize(void *stream)
{
	AGX_HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
	return AGX_OK;
}

} /* extern "C" */
