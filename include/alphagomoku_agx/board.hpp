/*
 * alphagomoku_agx/board.hpp — ag::Sign and ag::matrix, the board type of Tree::setBoard and AGNetwork::packInputData.
 */
#ifndef ALPHAGOMOKU_AGX_BOARD_HPP_
#define ALPHAGOMOKU_AGX_BOARD_HPP_

#include <cstddef>
#include <cstdint>
#include <vector>

namespace ag
{
	enum class Sign : int16_t
	{ // game/Move.hpp:17-23
		NONE, CROSS, CIRCLE, ILLEGAL
	};
	template<typename T>
	class matrix
	{ // utils/matrix.hpp: row-major rows x cols (the part of the interface the path's callers use)
			std::vector<T> m_data;
			int m_rows = 0, m_cols = 0;
		public:
			matrix() = default;
			matrix(int rows, int cols) :
					m_data(static_cast<size_t>(rows) * cols), m_rows(rows), m_cols(cols)
			{
			}
			int rows() const noexcept { return m_rows; }
			int cols() const noexcept { return m_cols; }
			int size() const noexcept { return m_rows * m_cols; }
			T* data() noexcept { return m_data.data(); }
			const T* data() const noexcept { return m_data.data(); }
			T& at(int r, int c) { return m_data.at(static_cast<size_t>(r) * m_cols + c); }
			const T& at(int r, int c) const { return m_data.at(static_cast<size_t>(r) * m_cols + c); }
			T& operator[](int i) noexcept { return m_data[i]; }
			const T& operator[](int i) const noexcept { return m_data[i]; }
			void fill(T value) { m_data.assign(m_data.size(), value); }
	};
} /* namespace ag */

#endif
